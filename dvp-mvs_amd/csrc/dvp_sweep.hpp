// dvp_sweep.hpp — the sweep site: DepthToWeak (APD.cu:3892-4051) and LocalRefine (APD.cu:4053-4139).
// First the per-pixel forms, which are the definition: depth_to_weak_px (REFINE: the same thread then does LocalRefine for
// its pixel) and local_refine_px.  Then the same launch site as view-compacted evaluation passes: sweep_prepare_px,
// sweep_eval_px, sweep_decide1_px, sweep_decide2_px.  From dvp_strong.hpp it takes the shared helpers only.
#ifndef DVP_SWEEP_HPP_
#define DVP_SWEEP_HPP_

#include "dvp_strong.hpp"

namespace dvp {

// shared prologue of DepthToWeak / LocalRefine (APD.cu:3928-3960, 4076-4108): cost at the current
// depth, mean baseline, weight sum over the selected views.
struct SweepCtx {
	f4 origin;          // camera-frame normal, .w = depth
	float depth;
	float cost_now, base_line, weight_normal;
	int valid;
	uint32_t sel;
};

// DepthToWeak (APD.cu:3892-4051).  REFINE: the same thread then does LocalRefine (APD.cu:4053-4139, the launch
// that follows, local_refine_px below) for its pixel.  LocalRefine's sweep slots -5..5 are planes the DepthToWeak
// sweep has just evaluated against the same views — same plane, same patch context, hence the same NCC and geometric
// costs bit for bit — so the fused kernel only folds them a second time in LocalRefine's own order
// ((ncc*w) + (factor*geom*w) per view) and adds LocalRefine's one extra slot, the current depth.  Neither kernel
// reads anything another pixel writes, so running them back to back per pixel is the two launches' result.
template <int SMP>
DVP_HD void local_refine_px(const Dev& d, int px, int py, PatchTab tab, unsigned long long* nevals);
template <int SMP, bool REFINE>
DVP_HD void depth_to_weak_px(const Dev& d, int px, int py, PatchTab tab, unsigned long long* nevals) {
	const int W = d.width, H = d.height;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	if (P.use_radius && d.radius[center] == 0) d.radius[center] = P.strong_radius;
	if (px < 6 || py < 6 || px >= W - 6 || py >= H - 6) {
		d.weak_info[center] = DVP_UNKNOWN;
		if (REFINE) local_refine_px<SMP>(d, px, py, tab, nevals);   // LocalRefine has no border rule
		return;
	}
	const f4 origin = normal_world_to_cam(rc, d.planes[center]);
	const float origin_depth = origin.w;
	if (origin_depth == 0) { d.weak_info[center] = DVP_UNKNOWN; return; }   // (LocalRefine returns here too)
	const uint32_t sel = d.selected_views[center];
	const uint8_t* vw = d.view_weight + (size_t)center * 32;
	PatchCtx c;
	{
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		build_patch_ctx(d, px, py, radius, inc, 0, tab, &c);
	}
	float base_line = 0, weight_normal = 0.0f;
	int valid = 0;
	for (int v = 0; v < S; ++v) {
		if (!is_set(sel, v)) continue;
		weight_normal += vw[v];
		const float c0 = rc.c[0] - d.cameras[v + 1].c[0];
		const float c1 = rc.c[1] - d.cameras[v + 1].c[1];
		const float c2 = rc.c[2] - d.cameras[v + 1].c[2];
		base_line += sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
		valid++;
	}
	if (valid == 0) { d.weak_info[center] = DVP_UNKNOWN; return; }   // (LocalRefine returns here too)
	base_line /= valid;
	const float disp = rc.K[0] * base_line / origin_depth;
	const bool refine = REFINE && weight_normal != 0;   // LocalRefine's own guard (APD.cu:4075)
	// the reference also evaluates cost_now at the current depth (APD.cu:3937-3941); its value
	// is never used by DepthToWeak, so those evaluations are not issued.
	float p_costs[61];
	float lr_costs[11];            // LocalRefine's total of sweep slot pd = -5..5
	unsigned lr_live = 0;          // ... bit pd+5: the slot is inside the depth range
	// Sweep order: the central window first.  A pixel is WEAK whenever there is no cost peak <= 0.5 within
	// weak_peak_radius of the current depth — either there is no peak at all (min_peak = 0), or the lowest peak lies outside
	// the window, or it lies inside with a cost above 0.5 (APD.cu:4018-4023) — and that is decided by the window and its two
	// neighbours alone: such pixels skip the other ~46 planes (exact: their costs cannot change the state, and LocalRefine
	// only reads the slots -5..5).  Textureless regions, i.e. most WEAK pixels, leave here.  One loop, one call site of the
	// evaluator: k walks the window (-cw..cw), then the planes left of it, then those right of it.
	int cw = P.weak_peak_radius + 1;
	if (cw < 5) cw = 5;
	if (cw > 30) cw = 30;
	bool central_peak = false;
	auto window_has_peak = [&]() {
		bool any = false;
		for (int i = 30 - P.weak_peak_radius; i <= 30 + P.weak_peak_radius; ++i) {
			if (i < 2 || i > 58) continue;
			if (p_costs[i - 1] > p_costs[i] && p_costs[i + 1] > p_costs[i] && !(p_costs[i] > 0.5f)) any = true;
		}
		return any;
	};
	for (int k = 0; k < 61; ++k) {
		if (k == 2 * cw + 1) {
			central_peak = window_has_peak();
			if (!central_peak) break;
		}
		const int pd = k <= 2 * cw ? k - cw : (k - (2 * cw + 1) < 30 - cw ? k - (2 * cw + 1) - 30 : k - 30);
		if (!sweep_slot_read(cw, pd, d.sweep_all_slots != 0)) { p_costs[pd + 30] = 2.0f; continue; }   // the two end slots: no decision reads them
		const float p_depth = rc.K[0] * base_line / (disp + pd);
		if (p_depth < P.depth_min || p_depth > P.depth_max) { p_costs[pd + 30] = 2.0f; continue; }
		f4 pl = origin;
		pl.w = distance_to_origin(rc, px, py, p_depth, pl);
		const bool both = refine && pd >= -5 && pd <= 5;
		f3 fwd;   // the plane's 3-D point, shared by the views' geometric terms
		if (P.geom_consistency) fwd = geom_forward_point(d, px, py, pl);
		float pc = 0.0f, lr = 0.0f;
		for (int v = 0; v < S; ++v) {
			if (!is_set(sel, v)) continue;
			// a selected view with zero weight contributes cost*0 = +0: skipped (finite cost)
			if (vw[v] == 0) continue;
			const float ncc = ncc_old<SMP>(d, c, px, py, v + 1, pl);
			if (nevals) *nevals += 1;
			const float gc = P.geom_consistency ? geom_cost_of_point(d, px, py, v + 1, fwd) : 0.0f;
			float cst = ncc;
			if (P.geom_consistency) cst += P.geom_factor * gc;
			const float tc = 0.0f + cst;
			pc += tc * vw[v];
			if (both) {   // ncc*w and (factor*geom)*w added separately, APD.cu:4124-4126
				lr += ncc * vw[v];
				if (P.geom_consistency) lr += (P.geom_factor * gc * vw[v]);
			}
		}
		pc /= weight_normal;
		p_costs[pd + 30] = DVP_MIN(2.0f, pc);
		if (both) { lr_costs[pd + 5] = lr / weight_normal; lr_live |= 1u << (pd + 5); }
	}
	if (cw == 30) central_peak = window_has_peak();
	uint64_t is_peak = 0;
	int peak_count = 0, min_peak = 0;
	float min_cost = 2.0f;
	for (int i = 2; central_peak && i < 59; ++i) {
		if (p_costs[i - 1] > p_costs[i] && p_costs[i + 1] > p_costs[i]) {
			is_peak |= (uint64_t)1 << i;
			peak_count++;
			if (p_costs[i] < min_cost) { min_peak = i; min_cost = p_costs[i]; }
		}
	}
	const int dpk = min_peak - 30;
	uint8_t state;
	if (!central_peak) state = DVP_WEAK;
	else if ((dpk < 0 ? -dpk : dpk) > P.weak_peak_radius || p_costs[min_peak] > 0.5f) state = DVP_WEAK;
	else if (peak_count == 1) state = (p_costs[min_peak] <= 0.15f) ? DVP_STRONG : DVP_WEAK;
	else {
		float var = 0.0f;
		for (int i = 2; i < 59; ++i) {
			if (((is_peak >> i) & 1) && i != min_peak) {
				const float dist = p_costs[i] - min_cost;
				var += dist * dist;
			}
		}
		var = sqrtf(var);
		var /= (peak_count - 1);
		state = (var > 0.2f) ? DVP_STRONG : DVP_WEAK;
	}
	d.weak_info[center] = state;
	if (!refine) return;
	// ---- LocalRefine: the current depth (cost_now, APD.cu:4080-4090), then the minimum over the sweep slots ----
	float cost_now = 0.0f;
	{
		f4 pl = origin;
		pl.w = distance_to_origin(rc, px, py, origin_depth, pl);
		for (int v = 0; v < S; ++v) {
			if (!is_set(sel, v)) continue;
			if (vw[v] == 0) continue;
			const float ncc = ncc_old<SMP>(d, c, px, py, v + 1, pl);
			if (nevals) *nevals += 1;
			float t = ncc;   // (ncc + factor*geom) * w, APD.cu:4085-4089
			if (P.geom_consistency) t += P.geom_factor * geom_cost(d, px, py, v + 1, pl);
			cost_now += t * vw[v];
		}
		cost_now /= weight_normal;
	}
	float lr_min = 2.0f;
	int best_pd = -6;
	for (int pd = -5; pd <= 5; ++pd) {
		if (!((lr_live >> (pd + 5)) & 1)) continue;
		if (lr_costs[pd + 5] < lr_min) { lr_min = lr_costs[pd + 5]; best_pd = pd; }
	}
	const float best_depth = (best_pd == -6) ? origin_depth : rc.K[0] * base_line / (disp + best_pd);
	if (cost_now - lr_min > 0.1) d.planes[center].w = best_depth;
}

// LocalRefine (APD.cu:4053-4139)
template <int SMP>
DVP_HD void local_refine_px(const Dev& d, int px, int py, PatchTab tab, unsigned long long* nevals) {
	const int W = d.width;
	const int center = px + py * W;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	const f4 origin = normal_world_to_cam(rc, d.planes[center]);
	const float origin_depth = origin.w;
	if (origin_depth == 0) return;
	const uint32_t sel = d.selected_views[center];
	const uint8_t* vw = d.view_weight + (size_t)center * 32;
	float base_line = 0, weight_normal = 0.0f;
	int valid = 0;
	for (int v = 0; v < S; ++v) {
		if (!is_set(sel, v)) continue;
		weight_normal += vw[v];
		const float c0 = rc.c[0] - d.cameras[v + 1].c[0];
		const float c1 = rc.c[1] - d.cameras[v + 1].c[1];
		const float c2 = rc.c[2] - d.cameras[v + 1].c[2];
		base_line += sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
		valid++;
	}
	if (weight_normal == 0 || valid == 0) return;
	PatchCtx c;
	{
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		build_patch_ctx(d, px, py, radius, inc, 0, tab, &c);
	}
	base_line /= valid;
	const float disp = rc.K[0] * base_line / origin_depth;
	float cost_now = 0.0f, min_cost = 2.0f, best_depth = origin_depth;
	// slot -6: the current depth (cost_now, APD.cu:4080-4090); slots -5..5: the sweep
	for (int pd = -6; pd <= 5; ++pd) {
		float p_depth = origin_depth;
		if (pd >= -5) {
			p_depth = rc.K[0] * base_line / (disp + pd);
			if (p_depth < P.depth_min || p_depth > P.depth_max) continue;
		}
		f4 pl = origin;
		pl.w = distance_to_origin(rc, px, py, p_depth, pl);
		float tc = 0.0f;
		for (int v = 0; v < S; ++v) {
			if (!is_set(sel, v)) continue;
			if (vw[v] == 0) continue;   // contributes +0 (finite costs)
			const float ncc = ncc_old<SMP>(d, c, px, py, v + 1, pl);
			if (nevals) *nevals += 1;
			const float gc = P.geom_consistency ? geom_cost(d, px, py, v + 1, pl) : 0.0f;
			if (pd == -6) {   // (ncc + factor*geom) * w, APD.cu:4085-4089
				float t = ncc;
				if (P.geom_consistency) t += P.geom_factor * gc;
				tc += t * vw[v];
			} else {          // ncc*w and (factor*geom)*w added separately, APD.cu:4124-4126
				tc += ncc * vw[v];
				if (P.geom_consistency) tc += (P.geom_factor * gc * vw[v]);
			}
		}
		tc /= weight_normal;
		if (pd == -6) cost_now = tc;
		else if (tc < min_cost) { min_cost = tc; best_depth = p_depth; }
	}
	if (cost_now - min_cost > 0.1) d.planes[center].w = best_depth;
}

// ---- DepthToWeak + LocalRefine as view-compacted evaluation passes --------------------------------------------------------
// depth_to_weak_px<SMP, true> above is the definition: one lane per pixel walks 61 (+1) planes x its selected views.  A wave
// of 64 pixels executes a view as soon as ONE lane selected it (6.4 views per pixel, 8.0 per wave at cfg3), every plane makes
// the workgroup cycle through all source images (125 B of HBM traffic per evaluation against 10.8 in dvp_strong_eval), and the
// cost line, the weights and the peak logic sit in the evaluator's register budget.  Same evaluations, same bits, as passes:
//   sweep_prepare_px   per pixel: validity, (camera-frame normal, depth), mean baseline, disparity, weight sum -> sweep_rec
//   sweep_eval_px      per (pixel, source view): the planes of one stage against ONE view — launched view by view over the
//                      pixels that selected the view with a weight > 0 (compacted into one list per view: dvp_sweep_eval_list,
//                      dvp_sweep_list.hpp; or tile by tile, DVP_SWEEP_LIST=0: dvp_sweep_eval), nothing live
//                      but the evaluator -> sweep_cost.  Stage 0: the central window (-cw..cw) and LocalRefine's extra slot
//                      (the current depth); stage 1: the rest of the line, only for pixels whose window holds a cost peak
//                      (the others are WEAK whatever the rest says: exact, see depth_to_weak_px).  Its end slots -30 and +30 are
//                      not evaluated: no decision reads them (dvp_forms.hpp: sweep_slot_read), 59 slots of the 61
//   sweep_decide1_px   per pixel: folds the window in the reference's view order, decides `central peak`, does LocalRefine
//                      (its slots -5..5 and the current depth are all stage 0)
//   sweep_decide2_px   per pixel with a central peak: folds the rest of the line, peak statistics -> weak_info
// Border pixels (DepthToWeak marks them UNKNOWN, LocalRefine has no border rule) go through the fused kernel.
constexpr int kSweepExtra = 72;     // sweep_cost field of the current depth: ncc + factor * geom (APD.cu:4085-4089)
// (kSweepFields, sweep_window and sweep_cost_floats: dvp_forms.hpp — the host's band arithmetic needs them too)
enum { SWF_VALID = 1, SWF_REFINE = 2, SWF_PEAK = 4 };
// sweep_cost, the per (view, field, pixel) record.  DVP_SWEEP_LAYOUT 1 (default): [group of 64 pixels][view][field][64] — the 73 fields
// of a (group, view) are 18.7 KB in a row: an evaluation launch (one view) fills them slot after slot, a decision pass reads a view's 50
// slots from 50 neighbouring 256-byte lines.  0: [view][field][pixel] (rounds 4-5): the same slots lie L floats apart — 9 x 50 streams
// 100 MB from each other per wave (dvp_sweep_decide2 read its 48 GB at 2.4 TB/s, profiles/pmc_r06.json).
#ifndef DVP_SWEEP_LAYOUT
#define DVP_SWEEP_LAYOUT 1
#endif
DVP_HD size_t sweep_field_stride(const Dev& d) {   // between field f and f + 1 of the same (view, pixel)
#if DVP_SWEEP_LAYOUT == 1
	(void)d;
	return 64;
#else
	return (size_t)d.width * (size_t)d.height;
#endif
}
DVP_HD size_t sweep_cost_index(const Dev& d, int v, int f, int center) {
#if DVP_SWEEP_LAYOUT == 1
	const int S = d.params.num_images - 1;
	const int rel = center - d.sweep_px0;   // (the band's first pixel; 0 when the buffer holds the whole image)
	return (((size_t)(rel >> 6) * S + v) * kSweepFields + (size_t)f) * 64 + (size_t)(rel & 63);
#else
	const size_t L = (size_t)d.width * (size_t)d.height;
	return ((size_t)v * kSweepFields + (size_t)f) * L + (size_t)center;
#endif
}
DVP_HD bool sweep_is_border(const Dev& d, int px, int py) { return px < 6 || py < 6 || px >= d.width - 6 || py >= d.height - 6; }

DVP_HD void sweep_prepare_px(const Dev& d, int px, int py) {
	const int W = d.width;
	const int center = px + py * W;
	const size_t L = (size_t)W * (size_t)d.height;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	if (P.use_radius && d.radius[center] == 0) d.radius[center] = P.strong_radius;
	f4 info = mk4(0.0f, 0.0f, 0.0f, 0.0f);   // .w: flags (as an integer value)
	d.sweep_rec[L + center] = info;
	if (sweep_is_border(d, px, py)) { d.weak_info[center] = DVP_UNKNOWN; return; }   // (+ LocalRefine: the fused kernel's border launch)
	const f4 origin = normal_world_to_cam(rc, d.planes[center]);
	if (origin.w == 0) { d.weak_info[center] = DVP_UNKNOWN; return; }
	const uint32_t sel = d.selected_views[center];
	const uint8_t* vw = d.view_weight + (size_t)center * 32;
	float base_line = 0, weight_normal = 0.0f;
	int valid = 0;
	for (int v = 0; v < S; ++v) {
		if (!is_set(sel, v)) continue;
		weight_normal += vw[v];
		const float c0 = rc.c[0] - d.cameras[v + 1].c[0];
		const float c1 = rc.c[1] - d.cameras[v + 1].c[1];
		const float c2 = rc.c[2] - d.cameras[v + 1].c[2];
		base_line += sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
		valid++;
	}
	if (valid == 0) { d.weak_info[center] = DVP_UNKNOWN; return; }
	base_line /= valid;
	const float disp = rc.K[0] * base_line / origin.w;
	d.sweep_rec[center] = origin;
	d.sweep_rec[L + center] = mk4(base_line, disp, weight_normal, (float)(SWF_VALID | (weight_normal != 0 ? SWF_REFINE : 0)));
}

// does (pixel, view v (0-based)) take part in stage `stage`?
DVP_HD bool sweep_go(const Dev& d, int center, int v, int stage) {
	const size_t L = (size_t)d.width * (size_t)d.height;
	const int flags = (int)d.sweep_rec[L + center].w;
	if (!(flags & (stage == 0 ? SWF_VALID : SWF_PEAK))) return false;
	return is_set(d.selected_views[center], v) && d.view_weight[(size_t)center * 32 + v] != 0;
}

// `cams`: the reference camera and the camera of view v + 1 ([0], [1]) where the caller keeps them (LDS), or null
// ALL: the two end slots are evaluated too (DVP_SWEEP_ALL_SLOTS: dvp_sweep_eval_all).  A template argument, so that the walk's bounds
// stay constants: with run-time bounds the compiler schedules the loop body worse by more than the two slots save.
template <int SMP, bool ALL = false>
DVP_HD void sweep_eval_px(const Dev& d, int px, int py, int v, int stage, PatchTab tab, unsigned long long* nevals, const DvpCamera* cams = nullptr) {
	const int W = d.width;
	const int center = px + py * W;
	const size_t L = (size_t)W * (size_t)d.height;
	const DvpParams& P = d.params;
	const DvpCamera rc_own = load_camera(d, 0);
	const DvpCamera& rc = cams ? cams[0] : rc_own;
	const f4 origin = d.sweep_rec[center];
	const f4 info = d.sweep_rec[L + center];
	const float base_line = info.x, disp = info.y;
	const bool refine = ((int)info.w & SWF_REFINE) != 0;
	PatchCtx c;
	{
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
#if defined(DVP_ABL_SWEEP_NO_TABLE)   // timing ablations (wrong results): where the launch site's time goes, profiles/r06_sweep_ablation.txt
		c.tab = tab; c.radius = radius; c.inc = inc; c.fast = 1; c.sum_ref = 1.0f; c.sum_ref_ref = 2.0f; c.wsum = 1.0f;
		for (int t = 0; t < kTaps * kTaps; ++t) tab.set(t, mk2(d.nb_cos, d.nb_sin * (float)t));   // (written, so the evaluator stays alive)
#else
		build_patch_ctx(d, px, py, radius, inc, 0, tab, &c);
#endif
	}
	const int cw = sweep_window(P);
	float* out = d.sweep_cost + sweep_cost_index(d, v, 0, center);
	const size_t FS = sweep_field_stride(d);
	// The end slots -30 and +30, which no decision reads, are stage 1's first and last k (sweep_slot_read: at cw == 30 they are in
	// stage 0 and stay): the walk loses them through its bounds, their fields stay unwritten
	constexpr int kEnds = (sweep_slot_read(5, -30, ALL) || sweep_slot_read(5, 30, ALL)) ? 0 : 1;   // (5: stage 1 exists below the clamp only, any cw < 30)
	const int k0 = stage == 0 ? 0 : 2 * cw + 1 + kEnds, k1 = stage == 0 ? 2 * cw + 1 + (refine ? 1 : 0) : 61 - kEnds;
	for (int k = k0; k < k1; ++k) {
		const bool extra = stage == 0 && k == 2 * cw + 1;   // LocalRefine's current-depth slot
		const int pd = k <= 2 * cw ? k - cw : (k - (2 * cw + 1) < 30 - cw ? k - (2 * cw + 1) - 30 : k - 30);
		float p_depth = origin.w;
		if (!extra) {
			p_depth = rc.K[0] * base_line / (disp + pd);
			if (p_depth < P.depth_min || p_depth > P.depth_max) continue;
		}
		f4 pl = origin;
		pl.w = distance_to_origin(rc, px, py, p_depth, pl);
		// the geometric term's depth-map fetch is issued before the NCC evaluation and used after it
		GeomFetch gf;
		const bool split_geom = P.geom_consistency && cams != nullptr;
#if !defined(DVP_ABL_SWEEP_NO_GEOM) && !defined(DVP_SWEEP_GEOM_AFTER)
		if (split_geom) gf = geom_cost_fetch(d, cams[0], cams[1], v + 1, px, py, pl);
#endif
#if defined(DVP_ABL_SWEEP_NO_EVAL)
		const float ncc = pl.w * 1e-3f;
#else
		const float ncc = ncc_old<SMP>(d, c, px, py, v + 1, pl);
#endif
		if (nevals) *nevals += 1;
#if defined(DVP_ABL_SWEEP_NO_GEOM)   // timing ablation (wrong results)
		const float gc = 0.0f;
#elif defined(DVP_SWEEP_GEOM_AFTER)   // round 5's order (A/B)
		const float gc = !P.geom_consistency ? 0.0f : (cams ? geom_cost_cams(d, cams[0], cams[1], v + 1, px, py, pl) : geom_cost(d, px, py, v + 1, pl));
#else
		const float gc = !P.geom_consistency ? 0.0f : (split_geom ? geom_cost_finish(cams[0], cams[1], px, py, gf) : geom_cost(d, px, py, v + 1, pl));
#endif
#if defined(DVP_ABL_SWEEP_NO_STORE)
		if (ncc + gc != d.nb_thresh * 1e30f) continue;   // (never equal; a runtime value, so nothing is folded away)
#endif
		if (extra) {
			float t = ncc;
			if (P.geom_consistency) t += P.geom_factor * gc;
			DVP_NT_STORE(1, &out[(size_t)kSweepExtra * FS], t);
		} else if (pd >= -5 && pd <= 5) {
			DVP_NT_STORE(1, &out[(size_t)(pd + 30) * FS], ncc);
			if (P.geom_consistency) DVP_NT_STORE(1, &out[(size_t)(61 + pd + 5) * FS], gc);
		} else {
			float cst = ncc;
			if (P.geom_consistency) cst += P.geom_factor * gc;
			DVP_NT_STORE(1, &out[(size_t)(pd + 30) * FS], cst);
		}
	}
}

// The decision passes fold the per-view costs of a slot in the reference's view order (APD.cu:3965-4005, 4110-4130):
// pc = sum over the selected views of (0 + cost) * weight.  View outside, slots inside (unrolled): the ~50 loads of one
// view are in flight together, and every slot's sum still receives its terms in view order — a slot-outside loop is one
// dependent round trip per (slot, view) (35 ms per cfg3 launch for 33 GB).
// fold of sweep slot pd over the views in the reference's order (APD.cu:3965-4005, 4110-4130): *pc = the DepthToWeak cost
// (not yet divided), *lr = LocalRefine's total of the same slot
DVP_HD void sweep_fold(const Dev& d, int center, int pd, uint32_t sel, const uint8_t* vw, bool both, float* pc_out, float* lr_out) {
	const DvpParams& P = d.params;
	const int S = P.num_images - 1;
	const size_t FS = sweep_field_stride(d);
	float pc = 0.0f, lr = 0.0f;
	for (int v = 0; v < S; ++v) {
		if (!is_set(sel, v)) continue;
		if (vw[v] == 0) continue;
		const float* in = d.sweep_cost + sweep_cost_index(d, v, 0, center);
		float ncc = 0.0f, gc = 0.0f, cst;
		if (pd >= -5 && pd <= 5) {
			ncc = DVP_NT_LOAD(2, &in[(size_t)(pd + 30) * FS]);
			cst = ncc;
			if (P.geom_consistency) { gc = DVP_NT_LOAD(2, &in[(size_t)(61 + pd + 5) * FS]); cst += P.geom_factor * gc; }
		} else {
			cst = DVP_NT_LOAD(2, &in[(size_t)(pd + 30) * FS]);
		}
		const float tc = 0.0f + cst;
		pc += tc * vw[v];
		if (both) {   // ncc*w and (factor*geom)*w added separately, APD.cu:4124-4126
			lr += ncc * vw[v];
			if (P.geom_consistency) lr += (P.geom_factor * gc * vw[v]);
		}
	}
	*pc_out = pc;
	*lr_out = lr;
}

DVP_HD void sweep_decide1_px(const Dev& d, int px, int py) {
	const int W = d.width;
	const int center = px + py * W;
	const size_t L = (size_t)W * (size_t)d.height;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	const f4 info = d.sweep_rec[L + center];
	const int flags = (int)info.w;
	if (!(flags & SWF_VALID)) return;
	const f4 origin = d.sweep_rec[center];
	const float base_line = info.x, disp = info.y, weight_normal = info.z;
	const bool refine = (flags & SWF_REFINE) != 0;
	const uint32_t sel = d.selected_views[center];
	const uint8_t* vw = d.view_weight + (size_t)center * 32;
	const int cw = sweep_window(P);
	float lr_costs[11];
	unsigned lr_live = 0;
	float cost_now = 0.0f;
#if !defined(DVP_SWEEP_FOLD_BRANCHY)
	if (cw == 5) {
		// The default window: the 11 slots are LocalRefine's too.  View outside, the view's 23 fields fetched together, the sums as
		// selects — every slot's sum still receives its terms in view order (sweep_fold below, slot outside with a load per (slot, view)
		// inside two branches, is the same arithmetic: 150 dependent round trips per pixel, 8.3 ms for 25 GB at cfg3).
		const size_t FS = sweep_field_stride(d);
		float pc[11], lr[11];
		unsigned in_range = 0;
#pragma unroll
		for (int i = 0; i < 11; ++i) {
			pc[i] = 0.0f; lr[i] = 0.0f;
			const float p_depth = rc.K[0] * base_line / (disp + (i - 5));
			if (!(p_depth < P.depth_min || p_depth > P.depth_max)) in_range |= 1u << i;
		}
		for (int v = 0; v < S; ++v) {
			if (!is_set(sel, v)) continue;
			if (vw[v] == 0) continue;
			const float* in = d.sweep_cost + sweep_cost_index(d, v, 0, center);
			const float w = vw[v];
			float ncc[11], gc[11];
#pragma unroll
			for (int i = 0; i < 11; ++i) {
				ncc[i] = DVP_NT_LOAD(2, &in[(size_t)(25 + i) * FS]);
				gc[i] = 0.0f;
				if (P.geom_consistency) gc[i] = DVP_NT_LOAD(2, &in[(size_t)(61 + i) * FS]);
			}
			const float extra = DVP_NT_LOAD(2, &in[(size_t)kSweepExtra * FS]);
			sched_fence();
#pragma unroll
			for (int i = 0; i < 11; ++i) {
				float cst = ncc[i];
				if (P.geom_consistency) cst += P.geom_factor * gc[i];
				const float tc = 0.0f + cst;
				const float t = pc[i] + tc * w;
				pc[i] = ((in_range >> i) & 1) ? t : pc[i];
				float u = lr[i] + ncc[i] * w;   // ncc*w and (factor*geom)*w added separately, APD.cu:4124-4126
				if (P.geom_consistency) u += (P.geom_factor * gc[i] * w);
				lr[i] = ((in_range >> i) & 1) ? u : lr[i];
			}
			const float cn = cost_now + extra * w;
			cost_now = refine ? cn : cost_now;
		}
#pragma unroll
		for (int i = 0; i < 11; ++i) {
			float pcv = 2.0f;
			if ((in_range >> i) & 1) {
				pcv = DVP_MIN(2.0f, pc[i] / weight_normal);
				if (refine) { lr_costs[i] = lr[i] / weight_normal; lr_live |= 1u << i; }
			}
			d.sweep_pc[(size_t)(25 + i) * L + center] = pcv;
		}
	} else
#endif
	{
	for (int pd = -cw; pd <= cw; ++pd) {
		const float p_depth = rc.K[0] * base_line / (disp + pd);
		float pcv = 2.0f;
		// (cw == 30: the end slots are in this window and stay, see sweep_slot_read)
		if (sweep_slot_read(cw, pd, d.sweep_all_slots != 0) && !(p_depth < P.depth_min || p_depth > P.depth_max)) {
			const bool both = refine && pd >= -5 && pd <= 5;
			float pc, lr;
			sweep_fold(d, center, pd, sel, vw, both, &pc, &lr);
			pc /= weight_normal;
			pcv = DVP_MIN(2.0f, pc);
			if (both) { lr_costs[pd + 5] = lr / weight_normal; lr_live |= 1u << (pd + 5); }
		}
		d.sweep_pc[(size_t)(pd + 30) * L + center] = pcv;
	}
	if (refine)
		for (int v = 0; v < S; ++v) {
			if (!is_set(sel, v)) continue;
			if (vw[v] == 0) continue;
			cost_now += d.sweep_cost[sweep_cost_index(d, v, kSweepExtra, center)] * vw[v];
		}
	}
	bool central_peak = false;
	for (int i = 30 - P.weak_peak_radius; i <= 30 + P.weak_peak_radius; ++i) {
		if (i < 2 || i > 58) continue;
		const float a = d.sweep_pc[(size_t)(i - 1) * L + center], b = d.sweep_pc[(size_t)i * L + center], e = d.sweep_pc[(size_t)(i + 1) * L + center];
		if (a > b && e > b && !(b > 0.5f)) central_peak = true;
	}
	if (!central_peak) d.weak_info[center] = DVP_WEAK;
	else d.sweep_rec[L + center].w = (float)(flags | SWF_PEAK);
	if (!refine) return;
	// ---- LocalRefine: the current depth (cost_now, APD.cu:4080-4090: summed with the folds above), then the minimum over the sweep slots ----
	cost_now /= weight_normal;
	float lr_min = 2.0f;
	int best_pd = -6;
	for (int pd = -5; pd <= 5; ++pd) {
		if (!((lr_live >> (pd + 5)) & 1)) continue;
		if (lr_costs[pd + 5] < lr_min) { lr_min = lr_costs[pd + 5]; best_pd = pd; }
	}
	const float best_depth = (best_pd == -6) ? origin.w : rc.K[0] * base_line / (disp + best_pd);
	if (cost_now - lr_min > 0.1) d.planes[center].w = best_depth;
}

// (the window is 11 slots at the default radius: the slot-outside fold of sweep_fold measures 8 ms per cfg3 launch, the unrolled
// view-outside form used below for the rest of the line 13 — 168 registers and a predicate per slot)
// CW: the window half-width known at compile time (5 at the default weak_peak_radius), 0 = read from the parameters.  With a run-time
// window every slot's `inside the window?` is a scalar branch around its load, and a wait at every join.
// ALL: the two end slots are fetched and folded too (DVP_SWEEP_ALL_SLOTS); otherwise their entries are the constant 2 (sweep_slot_read)
template <int CW, bool ALL>
DVP_HD void sweep_decide2_cw(const Dev& d, int px, int py) {
	const int W = d.width;
	const int center = px + py * W;
	const size_t L = (size_t)W * (size_t)d.height;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	const f4 info = d.sweep_rec[L + center];
	if (!((int)info.w & SWF_PEAK)) return;
	const float base_line = info.x, disp = info.y, weight_normal = info.z;
	const uint32_t sel = d.selected_views[center];
	const uint8_t* vw = d.view_weight + (size_t)center * 32;
	const int cw = CW > 0 ? CW : sweep_window(P);
	const size_t FS = sweep_field_stride(d);
	uint64_t live = 0;   // slots outside the window that are inside the depth range
	for (int pd = -30; pd <= 30; ++pd) {
		if ((pd >= -cw && pd <= cw) || !sweep_slot_read(cw, pd, ALL)) continue;
		const float p_depth = rc.K[0] * base_line / (disp + pd);
		if (!(p_depth < P.depth_min || p_depth > P.depth_max)) live |= (uint64_t)1 << (pd + 30);
	}
	float p_costs[61];
#pragma unroll
	for (int i = 0; i < 61; ++i) p_costs[i] = 0.0f;
	for (int v = 0; v < S; ++v) {
		if (!is_set(sel, v)) continue;
		if (vw[v] == 0) continue;
		const float* in = d.sweep_cost + sweep_cost_index(d, v, 0, center);
		const float w = vw[v];
		// every slot of the view is fetched — a slot outside the depth range holds whatever an earlier launch left, its sum is not
		// used — and the sums are selects, not branches: with `if (live) { load; add }` the compiler kept each load inside its branch
		// with a wait behind it, 50 dependent round trips per view (20.0 ms for 48 GB at cfg3, r06_kernel_stats; DVP_SWEEP_FOLD_BRANCHY)
		float cst[61];
#pragma unroll
		for (int i = 0; i < 61; ++i) {
			const int pd = i - 30;
			cst[i] = 0.0f;
			if (pd >= -cw && pd <= cw) continue;          // (uniform; cw >= 5: the slots with separate ncc / geom fields are all inside)
			if (!sweep_slot_read(cw, pd, ALL)) continue;      // (compile time at the default window)
#if defined(DVP_SWEEP_FOLD_BRANCHY)
			if ((live >> i) & 1)
#endif
			cst[i] = DVP_NT_LOAD(2, &in[(size_t)i * FS]);
		}
		sched_fence();
#pragma unroll
		for (int i = 0; i < 61; ++i) {
			const int pd = i - 30;
			if ((pd >= -cw && pd <= cw) || !sweep_slot_read(cw, pd, ALL)) continue;
			const float tc = 0.0f + cst[i];
			const float t = p_costs[i] + tc * w;
			p_costs[i] = ((live >> i) & 1) ? t : p_costs[i];
		}
	}
#pragma unroll
	for (int i = 0; i < 61; ++i) {
		const int pd = i - 30;
		if (!sweep_slot_read(cw, pd, ALL)) { p_costs[i] = 2.0f; continue; }
		if (pd >= -cw && pd <= cw) { p_costs[i] = d.sweep_pc[(size_t)i * L + center]; continue; }
		float q = p_costs[i] / weight_normal;
		q = DVP_MIN(2.0f, q);
		p_costs[i] = ((live >> i) & 1) ? q : 2.0f;
	}
	uint64_t is_peak = 0;
	int peak_count = 0, min_peak = 0;
	float min_cost = 2.0f;
#pragma unroll
	for (int i = 2; i < 59; ++i) {
		if (p_costs[i - 1] > p_costs[i] && p_costs[i + 1] > p_costs[i]) {
			is_peak |= (uint64_t)1 << i;
			peak_count++;
			if (p_costs[i] < min_cost) { min_peak = i; min_cost = p_costs[i]; }
		}
	}
	// p_costs[min_peak] == min_cost whenever a peak below 2 exists; otherwise min_peak = 0 and the line's first entry is read — which
	// cannot happen here (SWF_PEAK: the central peak <= 0.5 is a peak of this search too), so that entry may be the constant
	const float at_min = (min_peak == 0) ? p_costs[0] : min_cost;
	const int dpk = min_peak - 30;
	uint8_t state;
	if ((dpk < 0 ? -dpk : dpk) > P.weak_peak_radius || at_min > 0.5f) state = DVP_WEAK;
	else if (peak_count == 1) state = (at_min <= 0.15f) ? DVP_STRONG : DVP_WEAK;
	else {
		float var = 0.0f;
#pragma unroll
		for (int i = 2; i < 59; ++i) {
			if (((is_peak >> i) & 1) && i != min_peak) {
				const float dist = p_costs[i] - min_cost;
				var += dist * dist;
			}
		}
		var = sqrtf(var);
		var /= (peak_count - 1);
		state = (var > 0.2f) ? DVP_STRONG : DVP_WEAK;
	}
	d.weak_info[center] = state;
}
DVP_HD void sweep_decide2_px(const Dev& d, int px, int py) {
	if (d.sweep_all_slots) {
		if (sweep_window(d.params) == 5) sweep_decide2_cw<5, true>(d, px, py);
		else sweep_decide2_cw<0, true>(d, px, py);
	} else if (sweep_window(d.params) == 5) sweep_decide2_cw<5, false>(d, px, py);
	else sweep_decide2_cw<0, false>(d, px, py);
}

}  // namespace dvp
#endif
