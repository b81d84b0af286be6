// TEST INFRASTRUCTURE — the host emulation (tests/emul/emul.cpp, compiled into this library as it stands: same entry points, same
// device headers) plus the sweep site as view-compacted passes with the evaluation launches in the form the engine chooses
// (dvp_forms.hpp: sweep_eval_form): from per-view (pixel, view) lists, built by the functions the kernels share with the host
// (csrc/dvp_sweep_list.hpp) and consumed workgroup by workgroup in list order, or over the pixels (the engine's tile form).
// For tests/test_sweep_list_emul.py.
#include "../emul/emul.cpp"

namespace {
// what the last swl_run_passes with lists built for stage 1, i.e. from the flags its own dvp_sweep_decide1 left: the flags, the
// lengths and the lists one after the other (swl_stage1_lists)
std::vector<int> g_s1_flags, g_s1_len;
std::vector<uint32_t> g_s1_lists;
}  // namespace

extern "C" {

// DVP_SWEEP_ALL_SLOTS as the engine reads it when a context is created (dvp_ctx.hpp: sync_dev_struct)
void swl_read_switches(void* c) { ((Emu*)c)->d.sweep_all_slots = read_form_switches().sweep_all_slots ? 1 : 0; }

// dvp_engine.hip: launch_sweeps over the whole image.  Returns the evaluation launches' form (SweepEval), -1: the switches do not
// select the passes.  DVP_TEST_SWEEP_LIST_ALLOC_FAIL stands for lists that do not fit, as in the engine.
int swl_run_passes(void* c) {
	Emu& e = *(Emu*)c;
	const FormSwitches sw = read_form_switches();
	const SweepForm f = sweep_form(sw, true, e.d.params, true, e.W, e.H);
	if (f.kernel != SWEEP_PASSES) return -1;
	const SweepEval form = sweep_eval_form(sw, f, getenv("DVP_TEST_SWEEP_LIST_ALLOC_FAIL") == nullptr);
	const size_t L = (size_t)e.W * e.H;
	const int S = e.NI - 1;
	e.anchor_tab_valid = false;
	e.sweep_rec.assign(2 * L, mk4(0, 0, 0, 0));
	e.sweep_cost.assign(sweep_cost_floats(L, S), -7.0f);   // (a value no decision may ever read)
	e.sweep_pc.assign(61 * L, -7.0f);
	refresh(e);
	const int etx = (e.W + 63) / 64, tiles = etx * ((e.H + kSweepRows - 1) / kSweepRows), cap = (int)L;
	std::vector<uint32_t> list;
	std::vector<int> counts, len(S, 0);
	if (form == SWEEP_EVAL_LISTS) {
		list.assign((size_t)S * cap, 0xFFFFFFFFu);   // (a pixel outside every image)
		counts.assign((size_t)S * tiles, 0);
		e.d.sweep_list = list.data(); e.d.sweep_list_counts = counts.data(); e.d.sweep_list_n = len.data(); e.d.sweep_list_cap = cap;
	}
	const long long n = (long long)L;
	auto each_pixel = [&](auto&& fn) {
#pragma omp parallel for schedule(dynamic, 256)
		for (long long p = 0; p < n; ++p) fn((int)(p % e.W), (int)(p / e.W));
	};
	each_pixel([&](int px, int py) { sweep_prepare_px(e.d, px, py); });
	for (int stage = 0; stage < 2; ++stage) {
		if (stage == 1 && !f.second_eval) break;
		unsigned long long total = 0;
		// one lane of an evaluation launch: dvp_sweep_eval{,_exact}{,_all} / dvp_sweep_eval_list{,_exact}{,_all}
		auto eval_one = [&](int x, int y, int v) {
			unsigned long long k = 0;
			f2 tab_mem[kTaps * kTaps];
			const PatchTab tab{tab_mem, 1};
			unsigned long long* kp = e.count ? &k : nullptr;
			if (e.d.sweep_all_slots) {
				if (e.d.sampler) sweep_eval_px<1, true>(e.d, x, y, v, stage, tab, kp); else sweep_eval_px<0, true>(e.d, x, y, v, stage, tab, kp);
			} else if (e.d.sampler) sweep_eval_px<1, false>(e.d, x, y, v, stage, tab, kp);
			else sweep_eval_px<0, false>(e.d, x, y, v, stage, tab, kp);
			return k;
		};
		if (form == SWEEP_EVAL_LISTS) {
			// dvp_sweep_list_counts / dvp_scan3 / dvp_sweep_list_fill, then dvp_sweep_eval_list: every workgroup of the grid takes its chunk
			sweep_list_counts_host(e.d, etx, tiles, 0, stage, counts.data());
			sweep_list_scan_host(S, tiles, counts.data(), len.data());
			sweep_list_fill_host(e.d, etx, tiles, 0, stage, counts.data(), list.data(), cap);
			if (stage == 1) {
				g_s1_flags.resize(L);
				for (size_t p = 0; p < L; ++p) g_s1_flags[p] = (int)e.d.sweep_rec[L + p].w;
				g_s1_len = len;
				g_s1_lists.clear();
				for (int v = 0; v < S; ++v) g_s1_lists.insert(g_s1_lists.end(), list.begin() + (size_t)v * cap, list.begin() + (size_t)v * cap + len[v]);
			}
			const int grid = sweep_list_grid(cap, kSweepListRounds);
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : total) collapse(2)
			for (int v = 0; v < S; ++v)
				for (int b = 0; b < grid; ++b) {
					const int chunk = sweep_list_chunk(b, len[v], kSweepListRounds);
					if (chunk < 0) continue;
					const int first = chunk * 64 * kSweepListRounds, end = DVP_MIN(len[v], first + 64 * kSweepListRounds);
					for (int i = first; i < end; ++i) {
						const uint32_t ent = list[(size_t)v * cap + i];
						total += eval_one(sweep_list_x(ent), sweep_list_y(ent), v);
					}
				}
		} else {
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : total)
			for (long long p = 0; p < n; ++p)
				for (int v = 0; v < S; ++v)
					if (sweep_go(e.d, (int)p, v, stage)) total += eval_one((int)(p % e.W), (int)(p / e.W), v);
		}
		e.evals += total;
		if (stage == 0) each_pixel([&](int px, int py) { sweep_decide1_px(e.d, px, py); });
	}
	each_pixel([&](int px, int py) { sweep_decide2_px(e.d, px, py); });
	launch<kStageSweeps>(e, kSweepBorderOnly, 0);
	e.d.sweep_list = nullptr; e.d.sweep_list_counts = nullptr; e.d.sweep_list_n = nullptr; e.d.sweep_list_cap = 0;   // (the vectors end here)
	return (int)form;
}

// The stage-1 lists of the last swl_run_passes that built any, with the per-pixel flags (SWF_*) they were built from.  Sizes first
// (flags == nullptr): returns the total number of entries and fills len[S]; then the copies.  -1: none were built.
long long swl_stage1_lists(int S, int* len, int* flags, uint32_t* lists) {
	if ((int)g_s1_len.size() != S) return -1;
	for (int v = 0; v < S; ++v) len[v] = g_s1_len[v];
	if (flags) {
		std::memcpy(flags, g_s1_flags.data(), g_s1_flags.size() * sizeof(int));
		std::memcpy(lists, g_s1_lists.data(), g_s1_lists.size() * sizeof(uint32_t));
	}
	return (long long)g_s1_lists.size();
}

// field f of view v (0-based) of the passes' cost records as the last sweep site left them, one float per pixel; -1: no passes have run
int swl_sweep_field(void* c, int v, int f, float* dst) {
	Emu& e = *(Emu*)c;
	const size_t L = (size_t)e.W * e.H;
	if (v < 0 || v >= e.NI - 1 || f < 0 || f >= kSweepFields || e.sweep_cost.size() < sweep_cost_floats(L, e.NI - 1)) return -1;
	for (size_t p = 0; p < L; ++p) dst[p] = e.sweep_cost[sweep_cost_index(e.d, v, f, (int)p)];
	return 0;
}

// DVP_SWEEP_LIST and sweep_eval_form on their own (the lists of emu_forms_switches / emu_forms_decide are pinned by tests/test_forms.py).
// in: fused, geom, weak_peak_radius, sweep_fits, W, H, list_fits; out: the switch, the evaluation launches' form
void swl_forms_sweep_eval(const int* in, int* out) {
	const FormSwitches s = read_form_switches();
	DvpParams P;
	std::memset(&P, 0, sizeof(P));
	P.geom_consistency = in[1];
	P.weak_peak_radius = in[2];
	out[0] = s.sweep_list;
	out[1] = sweep_eval_form(s, sweep_form(s, in[0] != 0, P, in[3] != 0, in[4], in[5]), in[6] != 0);
}

}  // extern "C"
