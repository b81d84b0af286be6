// TEST INFRASTRUCTURE — the host emulation (tests/emul/emul.cpp, compiled into this library as it stands: same entry points, same
// device headers) plus what tests/test_sweep_dead_slots_host.py needs of the sweep site: DVP_SWEEP_ALL_SLOTS on the emulation, the
// engine's choice between dvp_sweep_eval and dvp_sweep_eval_all, and a look at the cost records the passes leave.
#include "../emul/emul.cpp"

extern "C" {

// the switch as the engine reads it when a context is created (dvp_ctx.hpp: sync_dev_struct); the emulation's own launches
// (emu_run_stage: the fused kernel, the separate kernels) then see it in Dev
void swh_read_switches(void* c) { ((Emu*)c)->d.sweep_all_slots = read_form_switches().sweep_all_slots ? 1 : 0; }

// the sweep site as view-compacted passes (dvp_engine.hip: launch_sweeps): emu_run_stage(kStageSweeps)'s sequence with the
// evaluation launch the engine picks under the switch
int swh_run_passes(void* c) {
	Emu& e = *(Emu*)c;
	const FormSwitches sw = read_form_switches();
	const SweepForm f = sweep_form(sw, true, e.d.params, true, e.W, e.H);
	if (f.kernel != SWEEP_PASSES) return -1;
	const bool all = e.d.sweep_all_slots != 0;
	const size_t L = (size_t)e.W * e.H;
	const int S = e.NI - 1;
	e.anchor_tab_valid = false;
	e.sweep_rec.assign(2 * L, mk4(0, 0, 0, 0));
	e.sweep_cost.assign(sweep_cost_floats(L, S), -7.0f);   // (a value no decision may ever read)
	e.sweep_pc.assign(61 * L, -7.0f);
	refresh(e);
	const long long n = (long long)L;
	auto each_pixel = [&](auto&& fn) {
#pragma omp parallel for schedule(dynamic, 256)
		for (long long p = 0; p < n; ++p) fn((int)(p % e.W), (int)(p / e.W));
	};
	each_pixel([&](int px, int py) { sweep_prepare_px(e.d, px, py); });
	for (int stage = 0; stage < 2; ++stage) {
		if (stage == 1 && !f.second_eval) break;
		unsigned long long total = 0;
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : total)
		for (long long p = 0; p < n; ++p)
			for (int v = 0; v < S; ++v) {
				if (!sweep_go(e.d, (int)p, v, stage)) continue;
				unsigned long long k = 0;
				f2 tab_mem[kTaps * kTaps];
				const PatchTab tab{tab_mem, 1};
				const int x = (int)(p % e.W), y = (int)(p / e.W);
				unsigned long long* kp = e.count ? &k : nullptr;
				if (all) {   // dvp_sweep_eval_all / dvp_sweep_eval_exact_all
					if (e.d.sampler) sweep_eval_px<1, true>(e.d, x, y, v, stage, tab, kp); else sweep_eval_px<0, true>(e.d, x, y, v, stage, tab, kp);
				} else if (e.d.sampler) sweep_eval_px<1, false>(e.d, x, y, v, stage, tab, kp);
				else sweep_eval_px<0, false>(e.d, x, y, v, stage, tab, kp);
				total += k;
			}
		e.evals += total;
		if (stage == 0) each_pixel([&](int px, int py) { sweep_decide1_px(e.d, px, py); });
	}
	each_pixel([&](int px, int py) { sweep_decide2_px(e.d, px, py); });
	launch<kStageSweeps>(e, kSweepBorderOnly, 0);
	return 0;
}

// field f of view v (0-based) of the passes' cost records as the last sweep site left them, one float per pixel; -1: no passes have run
int swh_sweep_field(void* c, int v, int f, float* dst) {
	Emu& e = *(Emu*)c;
	const size_t L = (size_t)e.W * e.H;
	if (v < 0 || v >= e.NI - 1 || f < 0 || f >= kSweepFields || e.sweep_cost.size() < sweep_cost_floats(L, e.NI - 1)) return -1;
	for (size_t p = 0; p < L; ++p) dst[p] = e.sweep_cost[sweep_cost_index(e.d, v, f, (int)p)];
	return 0;
}

}  // extern "C"
