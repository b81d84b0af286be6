// dvp_strong.hpp — per-pixel bodies of the strong path and the post-processing kernels: RandomInitialization, the strong
// update, GetDepthandNormal and the filter.  (DepthToWeak and LocalRefine: dvp_sweep.hpp.)
// One lane owns one pixel; a wave owns 64 x-adjacent pixels so that, once planes have locally
// converged, the 64 bilinear gathers of a tap hit a handful of 128-B lines.
#ifndef DVP_STRONG_HPP_
#define DVP_STRONG_HPP_

#include "dvp_ncc.hpp"

namespace dvp {

DVP_HD void sort_small(float* v, int n) {   // insertion sort, APD.cu:114-123
	for (int i = 1; i < n; i++) {
		const float tmp = v[i];
		int j = i;
		for (; j >= 1 && tmp < v[j - 1]; j--) v[j] = v[j - 1];
		v[j] = tmp;
	}
}

// GenerateRandomNormal_YZL (APD.cu:501-588): rejection-sample a unit normal that faces the
// reference viewing ray and the (quirkily transformed) viewing rays of every selected source view.
// `sel` = the pixel's selected-view mask (selected_views[center] at the time of the call)
DVP_HD f4 random_normal_yzl_sel(const Dev& d, int px, int py, Rng& rng, float depth, uint32_t sel) {
	const int W = d.width, H = d.height;
	const DvpCamera rc = load_camera(d, 0);
	f3 vd[20];
	{
		const f4 v0 = view_direction(rc, px, py, depth);
		vd[0] = mk3(v0.x, v0.y, v0.z);
	}
	int index = 1;
	for (int v = 1; v < d.params.num_images; ++v) {
		if (!is_set(sel, v - 1)) continue;
		const DvpCamera sc = load_camera(d, v);
		const f3 fwd = point_on_world((float)px, (float)py, depth, rc);
		f2 sp;
		float sd;
		project_on_camera(fwd, sc, &sp, &sd);
		const float sx = fminf(fmaxf(sp.x, -32768.0f), 32767.0f);
		const float sy = fminf(fmaxf(sp.y, -32768.0f), 32767.0f);
		const int ix = (int)((float)(int)sx + 0.5f), iy = (int)((float)(int)sy + 0.5f);   // APD.cu:525
		float src_depth = 1.0f;   // reference leaves it uninitialised outside the image (APD.cu:526)
		if (d.params.geom_consistency) {
			if (ix >= 0 && ix < W && iy >= 0 && iy < H)
				src_depth = tex_texel(d.depths + (size_t)v * d.plane_stride, d.org, d.pitch, W, H, (int)sx, (int)sy);
		}
		const f4 dir = view_direction(sc, ix, iy, src_depth);
		// R_c = R_ref * R_src^T ; R_f = R_c * {x, y, x} with row 2 using R_c[7] twice (APD.cu:14-18, 540-544)
		float Rc[9];
		for (int i = 0; i < 3; ++i)
			for (int j = 0; j < 3; ++j) {
				float acc = 0.0f;
				for (int k = 0; k < 3; ++k) acc += rc.R[i * 3 + k] * sc.R[j * 3 + k];
				Rc[i * 3 + j] = acc;
			}
		const float b0 = dir.x, b1 = dir.y, b2 = dir.x;
		const float f0 = Rc[0] * b0 + Rc[1] * b1 + Rc[2] * b2;
		const float f1 = Rc[3] * b0 + Rc[4] * b1 + Rc[5] * b2;
		const float f2_ = Rc[6] * b0 + Rc[7] * b1 + Rc[7] * b2;
		const float norm = sqrtf(f0 * f0 + f1 * f1 + f2_ * f2_);
		if (index < 20) vd[index++] = mk3(f0 / norm, f1 / norm, f2_ / norm);
	}
	int times = 200;
	f4 n = mk4(0, 0, 0, 0);
	while (times > 0) {
		float q1 = 1.0f, q2 = 1.0f, s = 2.0f;
		while (s >= 1.0f) {
			q1 = 2.0f * rng.uniform() - 1.0f;
			q2 = 2.0f * rng.uniform() - 1.0f;
			s = q1 * q1 + q2 * q2;
		}
		const float sq = sqrtf(1.0f - s);
		n.x = 2.0f * q1 * sq;
		n.y = 2.0f * q2 * sq;
		n.z = 1.0f - 2.0f * s;
		bool ok = true;
		for (int i = 0; i < index; i++) {
			const float dp = n.x * vd[i].x + n.y * vd[i].y + n.z * vd[i].z;
			if (dp > 0.0f) { ok = false; break; }
		}
		if (ok) break;
		times--;
	}
	normalize3(&n);
	return n;
}

DVP_HD f4 random_normal_yzl(const Dev& d, int px, int py, Rng& rng, float depth) {
	return random_normal_yzl_sel(d, px, py, rng, depth, d.selected_views[py * d.width + px]);
}

// The same draw for the split strong update's decision launch (S <= MV <= 16 views, unrolled).  random_normal_yzl_sel walks the
// views with `if (!selected) continue`, fetches the source depth of each inside that loop and appends to vd[index++]: one dependent
// round trip per selected view and a dynamically indexed private array (scratch) that the rejection loop re-reads on every try —
// half of dvp_strong_decide's 8.6 ms at cfg3 (timing ablation, profiles/r06_ab_notes.txt 20).  Here: the depth texels of all views
// fetched together (clamped addresses, the value used only where the reference reads it), the directions in registers behind a
// mask.  Same operations per selected view, same random numbers; the order in which a candidate is tested against the directions
// does not matter (it has to face away from all of them), and with at most 16 views the reference's limit of 19 never binds.
template <int MV>
DVP_HD f4 random_normal_yzl_views(const Dev& d, int px, int py, Rng& rng, float depth, uint32_t sel) {
	static_assert(MV <= 16, "the reference keeps at most 19 source directions (APD.cu:546)");
	const int W = d.width, H = d.height;
	const int S = d.params.num_images - 1;
	const DvpCamera rc = load_camera(d, 0);
	f3 vd0;
	{
		const f4 v0 = view_direction(rc, px, py, depth);
		vd0 = mk3(v0.x, v0.y, v0.z);
	}
	const f3 fwd = point_on_world((float)px, (float)py, depth, rc);
	int ixs[MV], iys[MV], txs[MV], tys[MV];
	float dep[MV];
	uint32_t inside = 0;
#pragma unroll
	for (int v = 1; v <= MV; ++v) {
		const int vv = v <= S ? v : S;   // (a view that exists; beyond S the result is not used)
		const DvpCamera sc = load_camera(d, vv);
		f2 sp;
		float sd;
		project_on_camera(fwd, sc, &sp, &sd);
		const float sx = fminf(fmaxf(sp.x, -32768.0f), 32767.0f);
		const float sy = fminf(fmaxf(sp.y, -32768.0f), 32767.0f);
		const int ix = (int)((float)(int)sx + 0.5f), iy = (int)((float)(int)sy + 0.5f);   // APD.cu:525
		ixs[v - 1] = ix; iys[v - 1] = iy;
		txs[v - 1] = (int)sx; tys[v - 1] = (int)sy;
		if (ix >= 0 && ix < W && iy >= 0 && iy < H) inside |= 1u << (v - 1);
	}
	if (d.params.geom_consistency) {   // (without it there are no depth planes)
#pragma unroll
		for (int v = 1; v <= MV; ++v) {
			const int vv = v <= S ? v : S;
			dep[v - 1] = tex_texel(d.depths + (size_t)vv * d.plane_stride, d.org, d.pitch, W, H, txs[v - 1], tys[v - 1]);   // (clamped inside tex_texel)
		}
	} else {
#pragma unroll
		for (int v = 1; v <= MV; ++v) dep[v - 1] = 1.0f;
	}
	sched_fence();
	f3 vd[MV];
	uint32_t valid = 0;
#pragma unroll
	for (int v = 1; v <= MV; ++v) {
		const int vv = v <= S ? v : S;
		const DvpCamera sc = load_camera(d, vv);
		float src_depth = 1.0f;   // reference leaves it uninitialised outside the image (APD.cu:526)
		if (d.params.geom_consistency && ((inside >> (v - 1)) & 1u)) src_depth = dep[v - 1];
		const f4 dir = view_direction(sc, ixs[v - 1], iys[v - 1], src_depth);
		float Rc[9];
		for (int i = 0; i < 3; ++i)
			for (int j = 0; j < 3; ++j) {
				float acc = 0.0f;
				for (int k = 0; k < 3; ++k) acc += rc.R[i * 3 + k] * sc.R[j * 3 + k];
				Rc[i * 3 + j] = acc;
			}
		const float b0 = dir.x, b1 = dir.y, b2 = dir.x;
		const float f0 = Rc[0] * b0 + Rc[1] * b1 + Rc[2] * b2;
		const float f1 = Rc[3] * b0 + Rc[4] * b1 + Rc[5] * b2;
		const float f2_ = Rc[6] * b0 + Rc[7] * b1 + Rc[7] * b2;
		const float norm = sqrtf(f0 * f0 + f1 * f1 + f2_ * f2_);
		vd[v - 1] = mk3(f0 / norm, f1 / norm, f2_ / norm);
		if (v <= S && is_set(sel, v - 1)) valid |= 1u << (v - 1);
	}
	int times = 200;
	f4 n = mk4(0, 0, 0, 0);
	while (times > 0) {
		float q1 = 1.0f, q2 = 1.0f, s = 2.0f;
		while (s >= 1.0f) {
			q1 = 2.0f * rng.uniform() - 1.0f;
			q2 = 2.0f * rng.uniform() - 1.0f;
			s = q1 * q1 + q2 * q2;
		}
		const float sq = sqrtf(1.0f - s);
		n.x = 2.0f * q1 * sq;
		n.y = 2.0f * q2 * sq;
		n.z = 1.0f - 2.0f * s;
		bool ok = !(n.x * vd0.x + n.y * vd0.y + n.z * vd0.z > 0.0f);
#pragma unroll
		for (int i = 0; i < MV; i++) {
			const float dp = n.x * vd[i].x + n.y * vd[i].y + n.z * vd[i].z;
			if (((valid >> i) & 1u) && dp > 0.0f) ok = false;
		}
		if (ok) break;
		times--;
	}
	normalize3(&n);
	return n;
}

// RandomInitialization (APD.cu:1273-1309)
template <int SMP>
DVP_HD void random_init_px(const Dev& d, int px, int py, PatchTab tab, unsigned long long* nevals) {
	const int center = py * d.width + px;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	f4 plane = d.planes[center];
	PatchCtx c;
	int radius, inc;
	patch_geometry(d, center, &radius, &inc);
	build_patch_ctx(d, px, py, radius, inc, 0, tab, &c);

	if (P.state == DVP_FIRST_INIT) {
		if (plane.w > P.depth_max || plane.w < P.depth_min) {
			// GenerateRandomPlaneHypothesis_YZL (APD.cu:663-669)
			Rng rd(d.seed, (uint32_t)center, rng_site(PH_RANDOM_INIT, 0, SUB_DEPTH_RAND));
			Rng rn(d.seed, (uint32_t)center, rng_site(PH_RANDOM_INIT, 0, SUB_NORMAL));
			const float depth = rd.uniform() * (P.depth_max - P.depth_min) + P.depth_min;
			plane = random_normal_yzl(d, px, py, rn, depth);
			plane.w = distance_to_origin(rc, px, py, depth, plane);
		}
		d.planes[center] = plane;
		// ComputeMultiViewInitialCostandSelectedViews (APD.cu:1115-1161)
		float cv[32], cvs[32];
		int valid = 0;
		for (int v = 0; v < S; ++v) {
			const float cst = ncc_old<SMP>(d, c, px, py, v + 1, plane);
			cv[v] = cst;
			cvs[v] = cst;
			if (cst < 2.0f) valid++;
		}
		if (nevals) *nevals += (unsigned long long)S;
		sort_small(cvs, S);
		uint32_t sel = 0;
		const int top_k = DVP_MIN(valid, P.top_k);
		float cost = 2.0f;
		if (top_k > 0) {
			float acc = 0.0f;
			for (int i = 0; i < top_k; ++i) acc += cvs[i];
			const float thr = cvs[top_k - 1];
			for (int i = 0; i < S; ++i)
				if (cv[i] <= thr) set_bit(&sel, i);
			cost = acc / top_k;
		}
		d.selected_views[center] = sel;
		d.costs[center] = cost;
	} else {
		plane = normal_world_to_cam(rc, plane);
		const float depth = plane.w;
		plane.w = distance_to_origin(rc, px, py, depth, plane);
		d.planes[center] = plane;
		// ComputeMultiViewInitialCost (APD.cu:1163-1194)
		uint32_t sel = d.selected_views[center];
		int cnt = 0;
		float acc = 0.0f;
		for (int v = 0; v < S; ++v) {
			if (!is_set(sel, v)) continue;
			const float cst = ncc_old<SMP>(d, c, px, py, v + 1, plane);
			if (nevals) *nevals += 1;
			if (cst < 2.0f) { cnt++; acc += cst; }
			else unset_bit_ref(&sel, v);
		}
		d.selected_views[center] = sel;
		d.costs[center] = (cnt == 0) ? 2.0f : acc / cnt;
	}
}

// Multi-hypothesis joint view selection (APD.cu:2483-2530 == 2803-2850)
template <int MV = 32>   // MV: row stride of cost_array and capacity of priors / vw (>= number of source views)
DVP_HD void joint_view_selection(const Dev& d, int center, int iter, int phase, const float* cost_array /*[8][MV]*/,
	const float* priors, uint8_t* vw /*[MV], zeroed*/, uint32_t* sel_mask, float* weight_norm) {
	const int S = d.params.num_images - 1;
	float probs[MV];
	const float thr = (float)(0.8 * dvp_expf((iter) * (iter) / (-90.0f)));
	for (int i = 0; i < S; i++) {
		float count = 0;
		int count_false = 0;
		float tmpw = 0;
		for (int j = 0; j < 8; j++) {
			const float cst = cost_array[j * MV + i];
			if (cst < thr) { tmpw += dvp_expf(cst * cst / (-0.18f)); count++; }
			if (cst > 1.2f) count_false++;
		}
		float pr = 0.0f;
		if (count > 2 && count_false < 3) pr = tmpw / count;
		else if (count_false < 3) pr = dvp_expf(thr * thr / (-0.32f));
		probs[i] = pr * priors[i];
	}
	// TransformPDFToCDF (APD.cu:356-370)
	float psum = 0.0f;
	for (int i = 0; i < S; ++i) psum += probs[i];
	const float inv = 1.0f / psum;
	float cum = 0.0f;
	for (int i = 0; i < S; ++i) { cum += probs[i] * inv; probs[i] = cum; }
	Rng rv(d.seed, (uint32_t)center, rng_site(phase, iter, SUB_VIEW));
	for (int s = 0; s < 15; ++s) {
		const float rp = rv.uniform() - FLT_EPSILON;
		for (int v = 0; v < S; ++v)
			if (probs[v] > rp) { vw[v] += 1; break; }
	}
	uint32_t m = 0;
	float wn = 0;
	for (int i = 0; i < S; ++i)
		if (vw[i] > 0) { set_bit(&m, i); wn += vw[i]; }
	*sel_mask = m;
	*weight_norm = wn;
}

// edge-adaptive sample search of one direction (APD.cu:2047-2081 / 2104-2118).
// pass 0: adaptive step; pass 1: 11 samples at stride 2.  Returns the position or -1.
DVP_HD int strong_sample_search(const Dev& d, int px, int py, int k, int pass) {
	const int W = d.width, H = d.height;
	const int center = py * W + px;
	const int dxs[8] = { 0, 0, -1, 1, -1, 1, -1, 1 };
	const int dys[8] = { -1, 1, 0, 0, -1, 1, 1, -1 };
	const int dx = dxs[k], dy = dys[k];
	int step_num = 11, step_len = 2;
	if (pass == 0) {
		const float max_edge_dist = DVP_MAX(H, W) / 30.0f;
		const s2 ep = d.edge_neigh[(size_t)center * 8 + k];
		const double ex = (double)(ep.x - px), ey = (double)(ep.y - py);
		float dist = (float)sqrt(ex * ex + ey * ey);
		if (k >= 4) dist = (float)((double)dist / sqrt(2.0));
		if (d.edge[center]) {
			dist = 22.0f;
		} else if (ep.y == -1 || dist >= max_edge_dist) {   // `!edge_pt.x == -1` is always false (APD.cu:2059)
			dist = max_edge_dist;
			if (k >= 4) dist = (float)((double)dist / sqrt(2.0));
		}
		step_num = DVP_MIN(DVP_MAX(11, (int)(1.0f * dist / 2)), 22);
		step_len = DVP_MAX((int)(1.0f * dist / step_num), 2);
		if (k < 4 && step_len % 2 == 1) step_len -= 1;
	}
	int fx = 0, fy = 0;
	if (k > 4) { if (k % 2) fx = dx; else fy = dy; }
	int best = -1;
	float min_cost = FLT_MAX;
	// step_num <= 22: fixed trip count with predicated loads so that all samples are in flight at
	// once instead of one dependent L2 round trip per sample
	float cs[22];
	int pcs[22];
#pragma unroll
	for (int step = 0; step < 22; ++step) {
		const int tx = px + 5 * dx + step * step_len * dx + fx;
		const int ty = py + 5 * dy + step * step_len * dy + fy;
		const bool ok = step < step_num && tx >= 0 && ty >= 0 && tx < W && ty < H;
		pcs[step] = ok ? tx + ty * W : -1;
		cs[step] = ok ? d.costs_snap[tx + ty * W] : 0.0f;
	}
#pragma unroll
	for (int step = 0; step < 22; ++step) {
		if (pcs[step] >= 0 && min_cost > cs[step]) { best = pcs[step]; min_cost = cs[step]; }
	}
	return (min_cost < FLT_MAX) ? best : -1;
}

// The sample positions of the 16 propagation slots of a pixel (8 edge-adaptive + 8 fixed, -1 = none)
// depend only on the pre-launch snapshot and the edge priors, so they are found by a separate,
// light launch (dozens of waves per SIMD hide the two dependent round trips per slot) and the
// register-starved update kernel reads one word per slot.
DVP_HD void strong_search_px(const Dev& d, int px, int py) {
	const int center = py * d.width + px;
	if (d.weak_info[center] == DVP_WEAK) return;
	const size_t L = (size_t)d.width * d.height;
	const bool is_edge = d.edge[center] != 0;
	for (int slot = 0; slot < 16; ++slot) {
		int pos = -1;
		if (slot < 8) pos = strong_sample_search(d, px, py, slot, 0);
		else if (!is_edge) pos = strong_sample_search(d, px, py, slot - 8, 1);
		d.search_pos[(size_t)slot * L + center] = pos;
	}
}

// CheckerboardPropagationStrong + PlaneHypothesisRefinementStrong
// (APD.cu:2010-2141, 2462-2567, 2725-2737, 1311-1383), use_edge branch.
//
// The 8 + 8 propagation candidates, the current plane and the 6 refinement hypotheses are walked
// by ONE loop with a single inlined copy of the 36-tap evaluation (23 "slots"); per slot a
// prologue picks the plane and the views to evaluate, an epilogue consumes the cost vector.
// After view selection only views with non-zero weight are evaluated: the reference evaluates all
// S and multiplies the others by a zero weight, which is the same value.
// MV = capacity of the per-view private arrays (cost_array[8][MV], cv, priors, vw): 32 covers
// every legal view count; the engine launches the MV = 8 instantiation when S <= 8, which keeps
// 1.2 KB/lane of zero-filled scratch out of the cache hierarchy (same values either way).
template <int SMP, int MV = 32>
DVP_HD void strong_update_px(const Dev& d, int px, int py, PatchTab tab, int iter, unsigned long long* nevals) {
	const int W = d.width;
	const int center = py * W + px;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	const uint32_t all_views = (S >= 32) ? 0xFFFFFFFFu : ((1u << S) - 1u);

	PatchCtx c;
	{
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		build_patch_ctx(d, px, py, radius, inc, 0, tab, &c);
	}
	float cost_array[8 * MV];
	for (int i = 0; i < 8 * MV; ++i) cost_array[i] = 0.0f;
	cost_array[0] = 2.0f;   // `= { 2.0f }` sets one element (APD.cu:2032)
	uint32_t flag = 0;      // bit k: direction k has a sample
	int positions[8];
	for (int k = 0; k < 8; ++k) positions[k] = 0;
	const bool is_edge = d.edge[center] != 0;
	const float good_thr = 0.8f * dvp_expf((iter) * (iter) / (-90.0f));

	uint8_t vw[MV];
	for (int i = 0; i < MV; ++i) vw[i] = 0;
	uint32_t sel_mask = 0;
	float weight_norm = 0.0f;
	float final_costs[8];
	int min_cost_idx = 0;
	float cost_now = 0.0f, costs_center = 0.0f, depth_now = 0.0f;
	f4 plane_now = mk4(0, 0, 0, 0);
	bool selected_views_written = false;
	// refinement hypotheses (APD.cu:1359-1360)
	float ref_depths[6];
	f4 ref_normals[6];

	float cv[MV];
	for (int slot = 0; slot < 23; ++slot) {
		// hypotheses 3 and 4 of the refinement are the same plane (both GeneratePerturbedNormal calls
		// return the input normal, APD.cu:1354-1360): the second one can never be accepted after the
		// first was tested (same cost, strict `<`), so it is not evaluated.
		if (slot == 21) continue;
		// ---- prologue: which plane, which views ----
		f4 plane = mk4(0, 0, 1, 1);
		uint32_t mask = 0;
		int pos = -1;
		if (slot < 16) {
			pos = d.search_pos[(size_t)slot * ((size_t)W * d.height) + center];   // strong_search_px (-1 on edge pixels for slots 8-15)
			if (pos >= 0) { plane = d.planes_snap[pos]; mask = all_views; }
		} else if (slot == 16) {
			// view selection (APD.cu:2462-2530)
			float priors[MV];
			for (int i = 0; i < MV; ++i) priors[i] = 0.0f;
			const int nb[4] = { center - W, center + W, center - 1, center + 1 };
			for (int i = 0; i < 4; ++i) {
				if ((flag >> (2 * i)) & 1) {   // guards flag[0],[2],[4],[6] (APD.cu:2471)
					const uint32_t sv = d.selected_views[nb[i]];
					for (int j = 0; j < S; ++j) priors[j] += is_set(sv, j) ? 0.9f : 0.1f;
				}
			}
			joint_view_selection<MV>(d, center, iter, PH_STRONG, cost_array, priors, vw, &sel_mask, &weight_norm);
			uint8_t* gvw = d.view_weight + (size_t)center * 32;
			for (int i = 0; i < 32; ++i) gvw[i] = i < MV ? vw[i < MV ? i : 0] : (uint8_t)0;
			for (int k = 0; k < 8; ++k) {
				float fc = 0.0f;
				for (int j = 0; j < S; ++j)
					if (vw[j] > 0) fc += vw[j] * cost_array[k * MV + j];
				final_costs[k] = fc / weight_norm;
			}
			min_cost_idx = 0;   // FindMinCostIndex (ties -> last, APD.cu:155-166)
			{
				float mc = final_costs[0];
				for (int k = 1; k < 8; ++k)
					if (final_costs[k] <= mc) { mc = final_costs[k]; min_cost_idx = k; }
			}
			plane = d.planes_snap[center];
			mask = sel_mask;
		} else {
			const int i = slot - 17;
			plane = ref_normals[i];
			plane.w = distance_to_origin(rc, px, py, ref_depths[i], plane);
			mask = sel_mask;
		}

		// ---- evaluate ----
		if (mask) {
			for (int v = 0; v < S; ++v) {
				if ((mask >> v) & 1) {
					cv[v] = ncc_old<SMP>(d, c, px, py, v + 1, plane);
					if (nevals) *nevals += 1;
				}
			}
		}

		// ---- epilogue ----
		if (slot < 8) {
			if (pos >= 0) {
				flag |= 1u << slot;
				positions[slot] = pos;
				for (int v = 0; v < S; ++v) cost_array[slot * MV + v] = cv[v];
			}
		} else if (slot < 16) {
			const int k = slot - 8;
			if (pos >= 0) {
				const bool had = (flag >> k) & 1;
				flag |= 1u << k;
				int good0 = 0, good1 = 0, bad0 = 0, bad1 = 0;
				for (int j = 0; j < S; ++j) {
					const float a = cost_array[k * MV + j], b = cv[j];
					if (a < good_thr) good0++;
					if (a > 1.2f) bad0++;
					if (b < good_thr) good1++;
					if (b > 1.2f) bad1++;
				}
				if (!had || good1 > good0 || (good1 == good0 && bad1 < bad0)) {
					positions[k] = pos;
					for (int j = 0; j < S; ++j) cost_array[k * MV + j] = cv[j];
				}
			}
		} else if (slot == 16) {
			// cost of the current plane under the new weights, adoption of the best neighbour
			// (APD.cu:2546-2567); a zero weight_norm makes everything NaN and every `<` false.
			float cn = 0.0f;
			for (int v = 0; v < S; ++v)
				if (vw[v] > 0) cn += vw[v] * cv[v];
			cost_now = cn / weight_norm;
			costs_center = cost_now;
			plane_now = d.planes_snap[center];
			depth_now = depth_from_plane(rc, plane_now, px, py);
			if ((flag >> min_cost_idx) & 1) {
				const f4 cand = d.planes_snap[positions[min_cost_idx]];
				const float db = depth_from_plane(rc, cand, px, py);
				if (db >= P.depth_min && db <= P.depth_max && final_costs[min_cost_idx] < cost_now) {
					depth_now = db;
					plane_now = cand;
					cost_now = final_costs[min_cost_idx];
					selected_views_written = true;
				}
			}
			// refinement hypotheses from the values at entry (APD.cu:1333-1360)
			Rng rd(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_DEPTH_RAND));
			Rng rn(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_NORMAL));
			Rng rp(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_DEPTH_PERT));
			const float depth_rand = rd.uniform() * (P.depth_max - P.depth_min) + P.depth_min;
			if (selected_views_written) d.selected_views[center] = sel_mask;   // read by random_normal_yzl
			const f4 n_rand = random_normal_yzl(d, px, py, rn, depth_now);
			const float dmin_p = (1 - 0.02f) * depth_now, dmax_p = (1 + 0.02f) * depth_now;
			const float depth_pert = rp.uniform() * (dmax_p - dmin_p) + dmin_p;
			f4 n_pert = plane_now;   // GeneratePerturbedNormal returns the normalised input (APD.cu:617-661)
			normalize3(&n_pert);
			ref_depths[0] = depth_rand; ref_normals[0] = plane_now;
			ref_depths[1] = depth_now;  ref_normals[1] = n_rand;
			ref_depths[2] = depth_rand; ref_normals[2] = n_rand;
			ref_depths[3] = depth_now;  ref_normals[3] = n_pert;
			ref_depths[4] = depth_now;  ref_normals[4] = n_pert;
			ref_depths[5] = depth_pert; ref_normals[5] = plane_now;
		} else {
			float tc = 0.0f;
			for (int j = 0; j < S; ++j)
				if (vw[j] > 0) tc += vw[j] * cv[j];
			tc /= weight_norm;
			const float db = depth_from_plane(rc, plane, px, py);
			if (db >= P.depth_min && db <= P.depth_max && tc < cost_now) {
				depth_now = db;
				plane_now = plane;
				cost_now = tc;
			}
		}
	}

	if (P.state == DVP_REFINE_INIT) {
		if (cost_now < costs_center - 0.1) {   // double comparison (APD.cu:2728)
			costs_center = cost_now;
			d.planes[center] = plane_now;
		}
	} else {
		costs_center = cost_now;
		d.planes[center] = plane_now;
	}
	d.costs[center] = costs_center;
}

// ===== split form of the strong update (engine launches only; same evaluations, same operations, same bits) ==========
// Measured on MI355X: the 36-tap evaluator alone runs at 32.7 G evaluations/s, inside the 23-slot loop of
// strong_update_px at 20-22, and the loop's decision logic alone (scratch-resident cost arrays, view selection, random
// normals at two waves per SIMD) costs 28 of the kernel's 109 ms.  The update is therefore issued as three launches:
//   dvp_strong_eval    strong_eval_px    the 16 propagation slots + the current plane, all S views each: pure functions of
//                                        the pre-launch snapshot; nothing live but the evaluator -> Dev::slot_costs
//   dvp_strong_decide  strong_decide_px  slot bookkeeping, view selection, adoption, refinement hypotheses: no evaluator,
//                                        no patch table, cost vectors in registers -> Dev::strong_rec (48 B per pixel)
//   dvp_strong_refine  strong_refine_px  the five refinement hypotheses against the selected views, acceptance, write-back
// strong_update_px stays the definition (host emulation, S > 16, dvp_run_stage A/B with DVP_STRONG_SPLIT=0).
constexpr int kSlotCur = 16;                 // slot_costs slot of the pixel's current plane
constexpr int kSlotCount = 17;
enum { SR_PLANE = 0, SR_DEPTH = 4, SR_COST = 5, SR_CENTER = 6, SR_DRAND = 7, SR_DPERT = 8, SR_NRAND = 9, SR_DUP = 12 /* 3 words: the place of every slot's vector, 5 bits each (strong_slot_place_of) */, SR_FIELDS = 15 };
DVP_HD size_t half_index(const Dev& d, int px, int py) { return (size_t)py * d.half_w + (size_t)(px >> 1); }
// Layout of Dev::slot_costs.  Round 6: [pixel of the colour][slot][view] — a pixel's 17 x S costs are one contiguous record.
// The evaluation launch's lanes are (pixel, slot) items, pixel-major: neighbouring lanes now write neighbouring 4 S-byte
// vectors (rounds 3-5, [slot][view][pixel]: 64 lines per store instruction), and a lane of the decision launch finds its 17 x S
// costs in five cache lines instead of 153 (strong update 466 -> 455 ms per cfg3 pass).
#ifndef DVP_SLOT_LAYOUT
#define DVP_SLOT_LAYOUT 1   // 0: [slot][view][pixel] (A/B)
#endif
// place of a slot's vector inside the pixel's record: the decision step takes the slots in pairs (k, 8 + k) — the adaptive and the
// fixed-stride sample of direction k — so the pairs lie side by side and a lane walks its record front to back, every cache line once
DVP_HD int slot_place(int slot) {
#if DVP_SLOT_LAYOUT
	return slot < 8 ? 2 * slot : (slot < 16 ? 2 * (slot - 8) + 1 : slot);
#else
	return slot;
#endif
}
DVP_HD size_t slot_cost_index(const Dev& d, int slot, int v, int px, int py) {
	const size_t Lh = (size_t)d.half_w * (size_t)d.height;
	const int S = d.params.num_images - 1;
#if DVP_SLOT_LAYOUT
	return (half_index(d, px, py) * kSlotCount + (size_t)slot_place(slot)) * (size_t)S + (size_t)v;
#else
	return (size_t)(slot * S + v) * Lh + half_index(d, px, py);
#endif
}
// where the decision step finds cost(slot, view) of its pixel: base[slot * slot_stride + view * view_stride]
struct SlotCostView { const float* base; size_t slot_stride, view_stride; };
DVP_HD SlotCostView slot_cost_view(const Dev& d, int px, int py) {
	const size_t Lh = (size_t)d.half_w * (size_t)d.height;
	const int S = d.params.num_images - 1;
	SlotCostView r;
#if DVP_SLOT_LAYOUT
	r.base = d.slot_costs + half_index(d, px, py) * kSlotCount * (size_t)S;
	r.slot_stride = (size_t)S;
	r.view_stride = 1;
#else
	r.base = d.slot_costs + half_index(d, px, py);
	r.slot_stride = (size_t)S * Lh;
	r.view_stride = Lh;
#endif
	return r;
}
// Round 4: the cost vector of a slot is a pure function of (pixel, plane), and the 17 planes of a pixel repeat — the
// edge-adaptive and the fixed search of a direction often end on the same pixel, and propagation itself makes neighbours
// carry bit-identical planes (11 % of the launch site's evaluations at cfg3).  Every bitwise-DISTINCT plane is evaluated
// once; a slot whose plane an earlier slot has already had is served by that slot's vector (same inputs through the same
// code: the same bits): src[slot] = the earliest slot with the same plane (itself when it is the first), 4 bits per slot in
// w[0] (slots 0-7) and w[1] (8-15), w[2] = src[16].  Returns the mask of the slots to evaluate.
DVP_HD bool same_plane_bits(const f4 a, const f4 b) {
	return f32_bits(a.x) == f32_bits(b.x) && f32_bits(a.y) == f32_bits(b.y) && f32_bits(a.z) == f32_bits(b.z) && f32_bits(a.w) == f32_bits(b.w);
}
// the 17 planes of a pixel's slots (a missing slot: zeros, bit clear in the returned mask)
DVP_HD uint32_t strong_slot_planes(const Dev& d, int center, f4 pl[kSlotCount]) {
	const size_t L = (size_t)d.width * d.height;
	uint32_t have = 0;
#pragma unroll
	for (int slot = 0; slot < kSlotCount; ++slot) {
		const int pos = slot < 16 ? d.search_pos[(size_t)slot * L + center] : center;
		pl[slot] = mk4(0.0f, 0.0f, 0.0f, 0.0f);
		if (pos >= 0) { pl[slot] = d.planes_snap[pos]; have |= 1u << slot; }
	}
	return have;
}
DVP_HD uint32_t strong_slot_sources_of(const f4 pl[kSlotCount], uint32_t have, uint32_t w[3]) {
	uint32_t uniq = 0;
	w[0] = w[1] = w[2] = 0;
#pragma unroll
	for (int slot = 0; slot < kSlotCount; ++slot) {
		int src = slot;
#pragma unroll
		for (int u = slot - 1; u >= 0; --u)     // ends with the EARLIEST equal slot, which is an evaluated one
			if (((have >> u) & 1u) && same_plane_bits(pl[u], pl[slot])) src = u;
		if (!((have >> slot) & 1u)) continue;
		if (src == slot) uniq |= 1u << slot;
		if (slot < 8) w[0] |= (uint32_t)src << (4 * slot);
		else if (slot < 16) w[1] |= (uint32_t)src << (4 * (slot - 8));
		else w[2] = (uint32_t)src;
	}
	return uniq;
}
DVP_HD uint32_t strong_slot_sources(const Dev& d, int center, uint32_t w[3]) {
	f4 pl[kSlotCount];
	const uint32_t have = strong_slot_planes(d, center, pl);
	return strong_slot_sources_of(pl, have, w);
}
DVP_HD int strong_slot_source(uint32_t w0, uint32_t w1, uint32_t w2, int slot) {
	return slot < 8 ? (int)((w0 >> (4 * slot)) & 15u) : slot < 16 ? (int)((w1 >> (4 * (slot - 8))) & 15u) : (int)w2;
}
// Round 8: the vector of a (pixel, plane) pair does not change inside the iteration loop either — it depends on the images,
// the cameras, the parameters, the sampler and the pixel's patch radius — and after the first iteration most neighbours still
// carry the plane they had at the pixel's previous visit.  With Dev::reuse_* set, every pixel of the FULL image keeps a record:
// 17 PLACES of S costs (reuse_costs), the plane of each place as raw bits (reuse_keys) and a header (valid places, radius,
// epoch).  The plan launch (dvp_strong_plan, next to the sample search) looks every distinct plane of the visit up among the
// valid keys, bitwise like same_plane_bits (-0 != +0, NaNs by payload).  A hit keeps its place and is not evaluated; a miss
// takes the lowest place no hit holds (17 places, at most 17 distinct planes: there always is one) and is evaluated into it.
// A record of another epoch or radius is empty.  Places no plane of this visit uses are dropped.
// The three SR_DUP words then carry the PLACE of every slot, 5 bits each, six slots per word.
constexpr uint32_t kPlaceMask = (1u << kSlotCount) - 1u;
DVP_HD int strong_slot_place_of(uint32_t w0, uint32_t w1, uint32_t w2, int slot) {
	return slot < 6 ? (int)((w0 >> (5 * slot)) & 31u) : slot < 12 ? (int)((w1 >> (5 * (slot - 6))) & 31u) : (int)((w2 >> (5 * (slot - 12))) & 31u);
}
// without the cache a slot's vector lies at the fixed place of its source slot (slot_place): the same words
DVP_HD void strong_source_places(const uint32_t src[3], uint32_t place_w[3]) {
	place_w[0] = place_w[1] = place_w[2] = 0;
#pragma unroll
	for (int s = 0; s < kSlotCount; ++s)
		place_w[s / 6] |= (uint32_t)slot_place(strong_slot_source(src[0], src[1], src[2], s)) << (5 * (s % 6));
}
DVP_HD PlaneKey plane_key(const f4 p) {
	PlaneKey k;
	k.w[0] = f32_bits(p.x); k.w[1] = f32_bits(p.y); k.w[2] = f32_bits(p.z); k.w[3] = f32_bits(p.w);
	return k;
}
// pl / have: strong_slot_planes; uniq / src: strong_slot_sources_of; keys: the pixel's 17 keys (read where the header says
// valid, written where a miss lands); hdr: read and rewritten.  Returns the slots to evaluate (also left in hdr->eval).
DVP_HD uint32_t strong_reuse_plan(const f4 pl[kSlotCount], uint32_t uniq, const uint32_t src[3], PlaneKey* keys, ReuseHdr* hdr,
                                  uint32_t epoch, int radius, uint32_t place_w[3]) {
	const ReuseHdr h = *hdr;
	const uint32_t valid = (h.epoch == epoch && h.radius == (uint32_t)radius) ? (h.valid & kPlaceMask) : 0u;
	int place[kSlotCount];
#pragma unroll
	for (int s = 0; s < kSlotCount; ++s) place[s] = -1;
	uint32_t held = 0;
	if (valid) {
#pragma unroll
		for (int p = 0; p < kSlotCount; ++p) {
			if (!((valid >> p) & 1u)) continue;
			const PlaneKey k = keys[p];
#pragma unroll
			for (int s = 0; s < kSlotCount; ++s) {
				if (!((uniq >> s) & 1u) || place[s] >= 0) continue;
				if (k.w[0] == f32_bits(pl[s].x) && k.w[1] == f32_bits(pl[s].y) && k.w[2] == f32_bits(pl[s].z) && k.w[3] == f32_bits(pl[s].w)) { place[s] = p; held |= 1u << p; }
			}
		}
	}
	uint32_t free_places = kPlaceMask & ~held, eval = 0;
#pragma unroll
	for (int s = 0; s < kSlotCount; ++s) {
		if (!((uniq >> s) & 1u) || place[s] >= 0) continue;
		const int p = dvp_ctz(free_places);
		free_places &= free_places - 1;
		place[s] = p;
		eval |= 1u << s;
		keys[p] = plane_key(pl[s]);
	}
	place_w[0] = place_w[1] = place_w[2] = 0;
#pragma unroll
	for (int s = 0; s < kSlotCount; ++s) {
		const int from = strong_slot_source(src[0], src[1], src[2], s);   // (a missing slot: 0; nobody reads its place)
		int p = 0;
#pragma unroll
		for (int u = 0; u <= s; ++u)
			if (u == from && place[u] >= 0) p = place[u];
		place_w[s / 6] |= (uint32_t)p << (5 * (s % 6));
	}
	ReuseHdr o;
	o.valid = kPlaceMask & ~free_places; o.radius = (uint32_t)radius; o.epoch = epoch; o.eval = eval;
	*hdr = o;
	return eval;
}
// the plan launch's lane: one non-WEAK pixel of the launch's colour
DVP_HD void strong_plan_px(const Dev& d, int px, int py) {
	const int center = py * d.width + px;
	f4 pl[kSlotCount];
	const uint32_t have = strong_slot_planes(d, center, pl);
	uint32_t src[3], pw[3];
	const uint32_t uniq = strong_slot_sources_of(pl, have, src);
	strong_reuse_plan(pl, uniq, src, d.reuse_keys + (size_t)center * kSlotCount, d.reuse_hdr + center, d.reuse_epoch, d.radius[center], pw);
	const size_t Lh = (size_t)d.half_w * (size_t)d.height;
	uint32_t* dup = reinterpret_cast<uint32_t*>(d.strong_rec) + half_index(d, px, py);
	dup[SR_DUP * Lh] = pw[0]; dup[(SR_DUP + 1) * Lh] = pw[1]; dup[(SR_DUP + 2) * Lh] = pw[2];
}
// one (pixel, slot) item: the slot's plane against all S views -> slot_costs
template <int SMP>
DVP_HD void strong_eval_item(const Dev& d, const PatchCtx& c, int px, int py, int slot, bool store, unsigned long long* nevals) {
	const int W = d.width;
	const int center = py * W + px;
	const int S = d.params.num_images - 1;
	const size_t L = (size_t)W * d.height;
	const int pos = slot < 16 ? d.search_pos[(size_t)slot * L + center] : center;
	const f4 plane = d.planes_snap[pos];
	// one loop for both record forms (a second inlined copy of the evaluator would cost the kernel its registers): `rec` = the
	// pixel's record, `at` = the vector's position in it — with the plane cache the slot's place in the pixel's own full-size record
	const bool reuse = d.reuse_costs != nullptr;
	float* const buf = reuse ? d.reuse_costs : d.slot_costs;
	int at = slot_place(slot);
	if (reuse) {
		const size_t Lh = (size_t)d.half_w * (size_t)d.height;
		const int word = (slot >= 6) + (slot >= 12);
		const uint32_t pw = reinterpret_cast<const uint32_t*>(d.strong_rec)[(size_t)(SR_DUP + word) * Lh + half_index(d, px, py)];
		at = (int)((pw >> (5 * (slot - 6 * word))) & 31u);
	}
	for (int v = 0; v < S; ++v) {
		const float cost = ncc_old<SMP>(d, c, px, py, v + 1, plane);
#if DVP_SLOT_LAYOUT
		const size_t rec = reuse ? (size_t)center : half_index(d, px, py);
		if (store) DVP_NT_STORE(4, &buf[(rec * kSlotCount + (size_t)at) * (size_t)S + (size_t)v], cost);
#else
		if (store) DVP_NT_STORE(4, &buf[reuse ? ((size_t)center * kSlotCount + (size_t)at) * (size_t)S + (size_t)v : slot_cost_index(d, slot, v, px, py)], cost);
#endif
	}
	if (nevals && store) *nevals += (unsigned long long)S;
}
// the pixel's share of the evaluation launch, one lane per pixel (the definition: host emulation, DVP_EVAL_ITEMS=0; the
// engine's default is the same items compacted over the lanes of a wave, dvp_strong_eval_items)
template <int SMP>
DVP_HD void strong_eval_px(const Dev& d, int px, int py, PatchTab tab, unsigned long long* nevals) {
	const int W = d.width;
	const int center = py * W + px;
	PatchCtx c;
	{
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		build_patch_ctx(d, px, py, radius, inc, 0, tab, &c);
	}
	uint32_t uniq;
	if (d.reuse_hdr) uniq = d.reuse_hdr[center].eval;   // the plan launch has listed the slots and written their places
	else {
		uint32_t src[3], w[3];
		uniq = strong_slot_sources(d, center, src);
		strong_source_places(src, w);
		const size_t Lh = (size_t)d.half_w * (size_t)d.height, hi = half_index(d, px, py);
		uint32_t* dup = reinterpret_cast<uint32_t*>(d.strong_rec) + hi;
		dup[SR_DUP * Lh] = w[0]; dup[(SR_DUP + 1) * Lh] = w[1]; dup[(SR_DUP + 2) * Lh] = w[2];
	}
	for (uint32_t m = uniq; m; m &= m - 1) strong_eval_item<SMP>(d, c, px, py, dvp_ctz(m), true, nevals);
}

// the S (<= MV) costs of one slot.  Pixel-major records hold them contiguously: 16-byte loads (4-byte aligned; the pieces beyond
// S belong to the next slot — the buffer carries 64 bytes of slack after the last record — and are not used)
template <int MV>
DVP_HD void load_slot_costs(const float* sc, size_t view_stride, int S, float* out) {
#if defined(__HIP_DEVICE_COMPILE__) && DVP_SLOT_LAYOUT
	typedef float f4v __attribute__((ext_vector_type(4), aligned(4)));
	constexpr int Q = (MV + 3) / 4;
	f4v q[Q];
#pragma unroll
	for (int i = 0; i < Q; ++i) q[i] = DVP_NT_LOAD(8, &reinterpret_cast<const f4v*>(sc)[i]);
#pragma unroll
	for (int v = 0; v < MV; ++v) out[v] = v < S ? q[v >> 2][v & 3] : 0.0f;
#else
#pragma unroll
	for (int v = 0; v < MV; ++v) out[v] = v < S ? sc[(size_t)v * view_stride] : 0.0f;
#endif
}

// Everything of strong_update_px between the propagation evaluations and the refinement evaluations, statement for
// statement, with the cost vectors in registers (all loops over directions / views are unrolled; MV >= S).
DVP_HD void strong_decide_wide_px(const Dev& d, int px, int py, int iter);
template <int MV>
DVP_HD void strong_decide_px(const Dev& d, int px, int py, int iter) {
#if !defined(__HIP_DEVICE_COMPILE__)
	// host builds only (the emulation dispatches on the bracket and knows none above 16): more views than the bracket holds are the
	// streaming form's.  No device instantiation carries this call.
	if (d.params.num_images - 1 > MV) { strong_decide_wide_px(d, px, py, iter); return; }
#endif
	const int W = d.width;
	const int center = py * W + px;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	// with the plane cache the vectors lie in the pixel's full-size record (strong_reuse_plan), else in the launch's half-size one;
	// either way the SR_DUP words give every slot's place in the record
	const bool reuse = d.reuse_costs != nullptr;
	SlotCostView cv;
	if (reuse) { cv.base = d.reuse_costs + (size_t)center * kSlotCount * (size_t)S; cv.slot_stride = (size_t)S; cv.view_stride = 1; }
	else cv = slot_cost_view(d, px, py);
	const size_t L = (size_t)W * d.height;
	const size_t Lh = (size_t)d.half_w * (size_t)d.height, hi = half_index(d, px, py);
	const float good_thr = 0.8f * dvp_expf((iter) * (iter) / (-90.0f));
	const uint32_t sel_entry = d.selected_views[center];   // (the pixel's own word: no other pixel of this colour writes it)
	float ca[8][MV];
	uint32_t flag = 0;
	int positions[8];
	// the place of every slot's vector (strong_source_places, written by the evaluation launch, or strong_reuse_plan's)
	const uint32_t* dup = reinterpret_cast<const uint32_t*>(d.strong_rec) + hi;
	const uint32_t dw0 = dup[SR_DUP * Lh], dw1 = dup[(SR_DUP + 1) * Lh], dw2 = dup[(SR_DUP + 2) * Lh];
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		positions[k] = 0;
#pragma unroll
		for (int v = 0; v < MV; ++v) ca[k][v] = 0.0f;
	}
	ca[0][0] = 2.0f;   // `= { 2.0f }` sets one element (APD.cu:2032)
	// The reference walks slots 0-7 (APD.cu:2047-2090) and then slots 8-15 (APD.cu:2104-2137); direction k of the second walk only
	// looks at what direction k of the first left, so the two are taken together here, direction by direction
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		{
			const int pos = d.search_pos[(size_t)k * L + center];
			if (pos >= 0) {
				flag |= 1u << k;
				positions[k] = pos;
				load_slot_costs<MV>(cv.base + (size_t)strong_slot_place_of(dw0, dw1, dw2, k) * cv.slot_stride, cv.view_stride, S, ca[k]);
			}
		}
		// slot 8 + k: the fixed-stride sample replaces the adaptive one if it is better
		const int pos = d.search_pos[(size_t)(8 + k) * L + center];
		if (pos >= 0) {
			const bool had = (flag >> k) & 1;
			flag |= 1u << k;
			float cb[MV];
			int good0 = 0, good1 = 0, bad0 = 0, bad1 = 0;
			load_slot_costs<MV>(cv.base + (size_t)strong_slot_place_of(dw0, dw1, dw2, 8 + k) * cv.slot_stride, cv.view_stride, S, cb);
#pragma unroll
			for (int j = 0; j < MV; ++j) {
				if (j < S) {
					const float a = ca[k][j], b = cb[j];
					if (a < good_thr) good0++;
					if (a > 1.2f) bad0++;
					if (b < good_thr) good1++;
					if (b > 1.2f) bad1++;
				}
			}
			if (!had || good1 > good0 || (good1 == good0 && bad1 < bad0)) {
				positions[k] = pos;
#pragma unroll
				for (int j = 0; j < MV; ++j)
					if (j < S) ca[k][j] = cb[j];
			}
		}
	}
	// ---- view selection (APD.cu:2462-2530), joint_view_selection on the register arrays ----
	float priors[MV];
#pragma unroll
	for (int i = 0; i < MV; ++i) priors[i] = 0.0f;
	{
		const int nb[4] = { center - W, center + W, center - 1, center + 1 };
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			if ((flag >> (2 * i)) & 1) {   // guards flag[0],[2],[4],[6] (APD.cu:2471)
				const uint32_t sv = d.selected_views[nb[i]];
#pragma unroll
				for (int j = 0; j < MV; ++j)
					if (j < S) priors[j] += is_set(sv, j) ? 0.9f : 0.1f;
			}
		}
	}
	float probs[MV];
	const float thr = (float)(0.8 * dvp_expf((iter) * (iter) / (-90.0f)));
#pragma unroll
	for (int i = 0; i < MV; ++i) {
		probs[i] = 0.0f;
		if (i < S) {
			float count = 0;
			int count_false = 0;
			float tmpw = 0;
#pragma unroll
			for (int j = 0; j < 8; j++) {
				const float cst = ca[j][i];
				if (cst < thr) { tmpw += dvp_expf(cst * cst / (-0.18f)); count++; }
				if (cst > 1.2f) count_false++;
			}
			float pr = 0.0f;
			if (count > 2 && count_false < 3) pr = tmpw / count;
			else if (count_false < 3) pr = dvp_expf(thr * thr / (-0.32f));
			probs[i] = pr * priors[i];
		}
	}
	float psum = 0.0f;
#pragma unroll
	for (int i = 0; i < MV; ++i)
		if (i < S) psum += probs[i];
	const float inv = 1.0f / psum;
	float cum = 0.0f;
#pragma unroll
	for (int i = 0; i < MV; ++i)
		if (i < S) { cum += probs[i] * inv; probs[i] = cum; }
	int vw[MV];
#pragma unroll
	for (int i = 0; i < MV; ++i) vw[i] = 0;
	Rng rv(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_VIEW));
	for (int s = 0; s < 15; ++s) {
		const float rp = rv.uniform() - FLT_EPSILON;
		bool done = false;
#pragma unroll
		for (int v = 0; v < MV; ++v)
			if (v < S && !done && probs[v] > rp) { vw[v] += 1; done = true; }
	}
	uint32_t sel_mask = 0;
	float weight_norm = 0;
#pragma unroll
	for (int i = 0; i < MV; ++i)
		if (i < S && vw[i] > 0) { set_bit(&sel_mask, i); weight_norm += vw[i]; }
	{
		uint8_t* gvw = d.view_weight + (size_t)center * 32;
		uint32_t words[8];
#pragma unroll
		for (int w8 = 0; w8 < 8; ++w8) {
			uint32_t x = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b)
				if (w8 * 4 + b < MV) x |= ((uint32_t)vw[w8 * 4 + b] & 255u) << (8 * b);
			words[w8] = x;
		}
		uint32_t* g32 = reinterpret_cast<uint32_t*>(gvw);   // 32-byte records: aligned
#pragma unroll
		for (int w8 = 0; w8 < 8; ++w8) g32[w8] = words[w8];
	}
	float final_costs[8];
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		float fc = 0.0f;
#pragma unroll
		for (int j = 0; j < MV; ++j)
			if (j < S && vw[j] > 0) fc += vw[j] * ca[k][j];
		final_costs[k] = fc / weight_norm;
	}
	int min_cost_idx = 0;   // FindMinCostIndex (ties -> last, APD.cu:155-166)
	{
		float mc = final_costs[0];
#pragma unroll
		for (int k = 1; k < 8; ++k)
			if (final_costs[k] <= mc) { mc = final_costs[k]; min_cost_idx = k; }
	}
	// ---- cost of the current plane under the new weights, adoption of the best neighbour (APD.cu:2546-2567) ----
	float cn = 0.0f;
#pragma unroll
	for (int v = 0; v < MV; ++v)
		if (v < S && vw[v] > 0) cn += vw[v] * cv.base[(size_t)strong_slot_place_of(dw0, dw1, dw2, kSlotCur) * cv.slot_stride + (size_t)v * cv.view_stride];
	float cost_now = cn / weight_norm;
	const float costs_center = cost_now;
	f4 plane_now = d.planes_snap[center];
	float depth_now = depth_from_plane(rc, plane_now, px, py);
	bool selected_views_written = false;
	{
		float fmin = final_costs[0];
		int pmin = positions[0];
#pragma unroll
		for (int k = 1; k < 8; ++k)
			if (k == min_cost_idx) { fmin = final_costs[k]; pmin = positions[k]; }
		if ((flag >> min_cost_idx) & 1) {
			const f4 cand = d.planes_snap[pmin];
			const float db = depth_from_plane(rc, cand, px, py);
			if (db >= P.depth_min && db <= P.depth_max && fmin < cost_now) {
				depth_now = db;
				plane_now = cand;
				cost_now = fmin;
				selected_views_written = true;
			}
		}
	}
	// ---- refinement hypotheses from the values at entry (APD.cu:1333-1360) ----
	Rng rd(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_DEPTH_RAND));
	Rng rn(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_NORMAL));
	Rng rp(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_DEPTH_PERT));
	const float depth_rand = rd.uniform() * (P.depth_max - P.depth_min) + P.depth_min;
	if (selected_views_written) d.selected_views[center] = sel_mask;   // (what random_normal_yzl reads)
#if defined(DVP_DECIDE_YZL_GENERIC)   // A/B: the per-view walk with its scratch array
	const f4 n_rand = random_normal_yzl(d, px, py, rn, depth_now);
#else
	const f4 n_rand = MV <= 16 ? random_normal_yzl_views<(MV <= 16 ? MV : 16)>(d, px, py, rn, depth_now, selected_views_written ? sel_mask : sel_entry)
	                           : random_normal_yzl(d, px, py, rn, depth_now);
#endif
	const float dmin_p = (1 - 0.02f) * depth_now, dmax_p = (1 + 0.02f) * depth_now;
	const float depth_pert = rp.uniform() * (dmax_p - dmin_p) + dmin_p;
	float* rec = d.strong_rec + hi;
	rec[(SR_PLANE + 0) * Lh] = plane_now.x; rec[(SR_PLANE + 1) * Lh] = plane_now.y; rec[(SR_PLANE + 2) * Lh] = plane_now.z; rec[(SR_PLANE + 3) * Lh] = plane_now.w;
	rec[SR_DEPTH * Lh] = depth_now; rec[SR_COST * Lh] = cost_now; rec[SR_CENTER * Lh] = costs_center;
	rec[SR_DRAND * Lh] = depth_rand; rec[SR_DPERT * Lh] = depth_pert;
	rec[(SR_NRAND + 0) * Lh] = n_rand.x; rec[(SR_NRAND + 1) * Lh] = n_rand.y; rec[(SR_NRAND + 2) * Lh] = n_rand.z;
}

// ===== the decision step for any S <= 31 (DVP_STRONG_WIDE, StrongForm::decide == 32): the cost vectors streamed, not held ========
// strong_decide_px keeps the eight directions' vectors in registers (8 x MV floats), which ends at MV = 16.  The decisions do not
// need them all at once.  Three passes over 16-byte pieces of four views, every piece found through the same place words:
//   A  per direction k: which of slot k and slot 8 + k gives the direction's vector.  The rule counts costs below good_thr and
//      above 1.2 over all views — integers, any order — and leaves two bits per direction (`flag`: a sample exists, `pick`: slot
//      8 + k's vector); the sample position is read again for the one direction that is adopted.  A direction without a sample
//      keeps the initialiser's vector, (2, 0, 0, ...) for k = 0 and zeros otherwise (wide_chosen_piece).
//   B  per view, in view order: the prior from the four neighbours' words (0.0f + 0.9f / 0.1f in neighbour order), the
//      eight-direction loop on element i of the chosen vectors in direction order -> probs[i].  CDF, draws and weights as in
//      strong_decide_px; the weights live packed as they are stored (view_weight, 8 words).
//   C  final_costs[k] and the current plane's cost: sums over the views in ascending order where the weight is > 0, multiply and
//      add rounded separately — the vectors are read a second time (L1 / L2), only the pieces that hold a selected view.
// Same operations on the same values in the same order per result as strong_decide_px / strong_update_px: the same bits.
constexpr int kWidePieces = 8;   // 4 views each
// views 4 q ... 4 q + 3 of the vector at `sc` (beyond S: 0), by value: the pieces stay in registers.  The caller asks for pieces with
// 4 q < S only: the 16 bytes end at most 12 bytes past the vector, inside the next one or the 64 bytes of slack behind the last record
DVP_HD f4 load_cost_piece(const float* sc, size_t view_stride, int S, int q) {
#if defined(__HIP_DEVICE_COMPILE__) && DVP_SLOT_LAYOUT
	typedef float f4v __attribute__((ext_vector_type(4), aligned(4)));
	const f4v v = reinterpret_cast<const f4v*>(sc)[q];
	return mk4(4 * q < S ? v[0] : 0.0f, 4 * q + 1 < S ? v[1] : 0.0f, 4 * q + 2 < S ? v[2] : 0.0f, 4 * q + 3 < S ? v[3] : 0.0f);
#else
	const float* p = sc + (size_t)(4 * q) * view_stride;
	return mk4(4 * q < S ? p[0] : 0.0f, 4 * q + 1 < S ? p[view_stride] : 0.0f, 4 * q + 2 < S ? p[2 * view_stride] : 0.0f, 4 * q + 3 < S ? p[3 * view_stride] : 0.0f);
#endif
}
DVP_HD float piece_view(const f4 p, int j) { return j == 0 ? p.x : (j == 1 ? p.y : (j == 2 ? p.z : p.w)); }   // (j: a constant after unrolling)
// acc + the piece's costs under the weights of its four views (a byte each in `w`), view by view where the weight is > 0
DVP_HD float wide_weighted_add(float acc, const f4 p, uint32_t w, int S, int q) {
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const int wv = (int)((w >> (8 * j)) & 255u);
		if (4 * q + j < S && wv > 0) acc += wv * piece_view(p, j);
	}
	return acc;
}
// piece q of direction k's vector after pass A
DVP_HD f4 wide_chosen_piece(const SlotCostView& cv, uint32_t dw0, uint32_t dw1, uint32_t dw2, uint32_t flag, uint32_t pick, int S, int k, int q) {
	f4 r = mk4((k == 0 && q == 0) ? 2.0f : 0.0f, 0.0f, 0.0f, 0.0f);   // no sample: the initialiser's vector, `= { 2.0f }` sets one element (APD.cu:2032)
	if ((flag >> k) & 1u) {
		const int slot = ((pick >> k) & 1u) ? 8 + k : k;
		r = load_cost_piece(cv.base + (size_t)strong_slot_place_of(dw0, dw1, dw2, slot) * cv.slot_stride, cv.view_stride, S, q);
	}
	return r;
}
DVP_HD void strong_decide_wide_px(const Dev& d, int px, int py, int iter) {
	const int W = d.width;
	const int center = py * W + px;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	const bool reuse = d.reuse_costs != nullptr;
	SlotCostView cv;
	if (reuse) { cv.base = d.reuse_costs + (size_t)center * kSlotCount * (size_t)S; cv.slot_stride = (size_t)S; cv.view_stride = 1; }
	else cv = slot_cost_view(d, px, py);
	const size_t L = (size_t)W * d.height;
	const size_t Lh = (size_t)d.half_w * (size_t)d.height, hi = half_index(d, px, py);
	const float good_thr = 0.8f * dvp_expf((iter) * (iter) / (-90.0f));
	const uint32_t sel_entry = d.selected_views[center];   // (the pixel's own word: no other pixel of this colour writes it)
	const uint32_t* dup = reinterpret_cast<const uint32_t*>(d.strong_rec) + hi;
	const uint32_t dw0 = dup[SR_DUP * Lh], dw1 = dup[(SR_DUP + 1) * Lh], dw2 = dup[(SR_DUP + 2) * Lh];
	uint32_t have = 0;   // bit s: slot s has a sample
#pragma unroll
	for (int slot = 0; slot < 16; ++slot)
		if (d.search_pos[(size_t)slot * L + center] >= 0) have |= 1u << slot;
	// ---- pass A: slot k or slot 8 + k (APD.cu:2047-2090, 2104-2137) ----
	uint32_t flag = 0, pick = 0;
#pragma unroll 1
	for (int k = 0; k < 8; ++k) {
		const bool h0 = (have >> k) & 1u, h1 = (have >> (8 + k)) & 1u;
		if (h0 || h1) flag |= 1u << k;
		if (h1 && !h0) pick |= 1u << k;
		if (h0 && h1) {   // the fixed-stride sample replaces the adaptive one if it is better
			const float* va = cv.base + (size_t)strong_slot_place_of(dw0, dw1, dw2, k) * cv.slot_stride;
			const float* vb = cv.base + (size_t)strong_slot_place_of(dw0, dw1, dw2, 8 + k) * cv.slot_stride;
			int good0 = 0, good1 = 0, bad0 = 0, bad1 = 0;
#pragma unroll
			for (int q = 0; q < kWidePieces; ++q) {
				if (4 * q < S) {
					const f4 pa = load_cost_piece(va, cv.view_stride, S, q), pb = load_cost_piece(vb, cv.view_stride, S, q);
#pragma unroll
					for (int j = 0; j < 4; ++j) {
						if (4 * q + j < S) {
							const float a = piece_view(pa, j), b = piece_view(pb, j);
							if (a < good_thr) good0++;
							if (a > 1.2f) bad0++;
							if (b < good_thr) good1++;
							if (b > 1.2f) bad1++;
						}
					}
				}
			}
			if (good1 > good0 || (good1 == good0 && bad1 < bad0)) pick |= 1u << k;
		}
	}
	// ---- pass B: view selection (APD.cu:2462-2530) ----
	uint32_t nbv[4];
	{
		const int nb[4] = { center - W, center + W, center - 1, center + 1 };
#pragma unroll
		for (int i = 0; i < 4; ++i) nbv[i] = ((flag >> (2 * i)) & 1u) ? d.selected_views[nb[i]] : 0u;   // guards flag[0],[2],[4],[6] (APD.cu:2471)
	}
	float probs[4 * kWidePieces];
	const float thr = (float)(0.8 * dvp_expf((iter) * (iter) / (-90.0f)));
#pragma unroll
	for (int q = 0; q < kWidePieces; ++q) {
#pragma unroll
		for (int j = 0; j < 4; ++j) probs[4 * q + j] = 0.0f;
		if (4 * q < S) {
			// the eight-direction loop of every view of the piece, direction by direction: a view's sums see the directions in order
			float count[4], tmpw[4];
			int count_false[4];
#pragma unroll
			for (int j = 0; j < 4; ++j) { count[j] = 0; tmpw[j] = 0; count_false[j] = 0; }
#pragma unroll
			for (int k = 0; k < 8; k++) {
				const f4 p = wide_chosen_piece(cv, dw0, dw1, dw2, flag, pick, S, k, q);
#pragma unroll
				for (int j = 0; j < 4; ++j) {
					const float cst = piece_view(p, j);
					if (cst < thr) { tmpw[j] += dvp_expf(cst * cst / (-0.18f)); count[j]++; }
					if (cst > 1.2f) count_false[j]++;
				}
			}
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const int i = 4 * q + j;
				if (i < S) {
					float prior = 0.0f;
#pragma unroll
					for (int n = 0; n < 4; ++n)
						if ((flag >> (2 * n)) & 1u) prior += is_set(nbv[n], i) ? 0.9f : 0.1f;
					float pr = 0.0f;
					if (count[j] > 2 && count_false[j] < 3) pr = tmpw[j] / count[j];
					else if (count_false[j] < 3) pr = dvp_expf(thr * thr / (-0.32f));
					probs[i] = pr * prior;
				}
			}
		}
	}
	float psum = 0.0f;
#pragma unroll
	for (int i = 0; i < 4 * kWidePieces; ++i)
		if (i < S) psum += probs[i];
	const float inv = 1.0f / psum;
	float cum = 0.0f;
#pragma unroll
	for (int i = 0; i < 4 * kWidePieces; ++i)
		if (i < S) { cum += probs[i] * inv; probs[i] = cum; }
	uint32_t words[kWidePieces];   // the weights, a byte per view (at most 15 each)
#pragma unroll
	for (int q = 0; q < kWidePieces; ++q) words[q] = 0;
	Rng rv(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_VIEW));
	for (int s = 0; s < 15; ++s) {
		const float rp = rv.uniform() - FLT_EPSILON;
		bool done = false;
#pragma unroll
		for (int v = 0; v < 4 * kWidePieces; ++v)
			if (v < S && !done && probs[v] > rp) { words[v >> 2] += 1u << (8 * (v & 3)); done = true; }
	}
	uint32_t sel_mask = 0;
	float weight_norm = 0;
#pragma unroll
	for (int i = 0; i < 4 * kWidePieces; ++i) {
		const int wv = (int)((words[i >> 2] >> (8 * (i & 3))) & 255u);
		if (i < S && wv > 0) { set_bit(&sel_mask, i); weight_norm += wv; }
	}
	{
		uint32_t* g32 = reinterpret_cast<uint32_t*>(d.view_weight + (size_t)center * 32);   // 32-byte records: aligned
#pragma unroll
		for (int q = 0; q < kWidePieces; ++q) g32[q] = words[q];
	}
	// ---- pass C: the eight directions' and the current plane's cost under the new weights ----
	float final_costs[8], cn = 0.0f;
#pragma unroll
	for (int k = 0; k < 8; ++k) final_costs[k] = 0.0f;
	{
		const float* cur = cv.base + (size_t)strong_slot_place_of(dw0, dw1, dw2, kSlotCur) * cv.slot_stride;
#pragma unroll
		for (int q = 0; q < kWidePieces; ++q) {
			if (4 * q < S && words[q] != 0) {
#pragma unroll
				for (int k = 0; k < 8; ++k) final_costs[k] = wide_weighted_add(final_costs[k], wide_chosen_piece(cv, dw0, dw1, dw2, flag, pick, S, k, q), words[q], S, q);
				cn = wide_weighted_add(cn, load_cost_piece(cur, cv.view_stride, S, q), words[q], S, q);
			}
		}
	}
#pragma unroll
	for (int k = 0; k < 8; ++k) final_costs[k] = final_costs[k] / weight_norm;
	int min_cost_idx = 0;   // FindMinCostIndex (ties -> last, APD.cu:155-166)
	{
		float mc = final_costs[0];
#pragma unroll
		for (int k = 1; k < 8; ++k)
			if (final_costs[k] <= mc) { mc = final_costs[k]; min_cost_idx = k; }
	}
	// ---- adoption of the best neighbour (APD.cu:2546-2567) ----
	float cost_now = cn / weight_norm;
	const float costs_center = cost_now;
	f4 plane_now = d.planes_snap[center];
	float depth_now = depth_from_plane(rc, plane_now, px, py);
	bool selected_views_written = false;
	{
		float fmin = final_costs[0];
#pragma unroll
		for (int k = 1; k < 8; ++k)
			if (k == min_cost_idx) fmin = final_costs[k];
		if ((flag >> min_cost_idx) & 1u) {
			const int slot = ((pick >> min_cost_idx) & 1u) ? 8 + min_cost_idx : min_cost_idx;
			const f4 cand = d.planes_snap[d.search_pos[(size_t)slot * L + center]];   // positions[min_cost_idx]
			const float db = depth_from_plane(rc, cand, px, py);
			if (db >= P.depth_min && db <= P.depth_max && fmin < cost_now) {
				depth_now = db;
				plane_now = cand;
				cost_now = fmin;
				selected_views_written = true;
			}
		}
	}
	// ---- refinement hypotheses from the values at entry (APD.cu:1333-1360) ----
	Rng rd(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_DEPTH_RAND));
	Rng rn(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_NORMAL));
	Rng rp(d.seed, (uint32_t)center, rng_site(PH_STRONG, iter, SUB_DEPTH_PERT));
	const float depth_rand = rd.uniform() * (P.depth_max - P.depth_min) + P.depth_min;
	if (selected_views_written) d.selected_views[center] = sel_mask;
	// the generic walk: it carries the reference's limit of 19 source directions (`if (index < 20)`), which binds from 20 mask bits on
	const f4 n_rand = random_normal_yzl_sel(d, px, py, rn, depth_now, selected_views_written ? sel_mask : sel_entry);
	const float dmin_p = (1 - 0.02f) * depth_now, dmax_p = (1 + 0.02f) * depth_now;
	const float depth_pert = rp.uniform() * (dmax_p - dmin_p) + dmin_p;
	float* rec = d.strong_rec + hi;
	rec[(SR_PLANE + 0) * Lh] = plane_now.x; rec[(SR_PLANE + 1) * Lh] = plane_now.y; rec[(SR_PLANE + 2) * Lh] = plane_now.z; rec[(SR_PLANE + 3) * Lh] = plane_now.w;
	rec[SR_DEPTH * Lh] = depth_now; rec[SR_COST * Lh] = cost_now; rec[SR_CENTER * Lh] = costs_center;
	rec[SR_DRAND * Lh] = depth_rand; rec[SR_DPERT * Lh] = depth_pert;
	rec[(SR_NRAND + 0) * Lh] = n_rand.x; rec[(SR_NRAND + 1) * Lh] = n_rand.y; rec[(SR_NRAND + 2) * Lh] = n_rand.z;
}

// PlaneHypothesisRefinementStrong's evaluations and acceptance (APD.cu:1361-1383) + the write-back (APD.cu:2725-2737)
template <int SMP, bool LANE_WALK = false>
DVP_HD void strong_refine_px(const Dev& d, int px, int py, PatchTab tab, unsigned long long* nevals) {
	const int W = d.width;
	const int center = py * W + px;
	const DvpParams& P = d.params;
	const DvpCamera rc = load_camera(d, 0);
	const int S = P.num_images - 1;
	const size_t Lh = (size_t)d.half_w * (size_t)d.height, hi = half_index(d, px, py);
	PatchCtx c;
	{
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		build_patch_ctx(d, px, py, radius, inc, 0, tab, &c);
	}
	const float* rec = d.strong_rec + hi;
	f4 plane_now = mk4(rec[(SR_PLANE + 0) * Lh], rec[(SR_PLANE + 1) * Lh], rec[(SR_PLANE + 2) * Lh], rec[(SR_PLANE + 3) * Lh]);
	float depth_now = rec[SR_DEPTH * Lh], cost_now = rec[SR_COST * Lh], costs_center = rec[SR_CENTER * Lh];
	const float depth_rand = rec[SR_DRAND * Lh], depth_pert = rec[SR_DPERT * Lh];
	const f4 n_rand = mk4(rec[(SR_NRAND + 0) * Lh], rec[(SR_NRAND + 1) * Lh], rec[(SR_NRAND + 2) * Lh], 0.0f);
	f4 n_pert = plane_now;   // GeneratePerturbedNormal returns the normalised input (APD.cu:617-661)
	normalize3(&n_pert);
	// view weights of this launch (strong_decide_px wrote them): two 16-byte loads
	const uint32_t* g32 = reinterpret_cast<const uint32_t*>(d.view_weight + (size_t)center * 32);
	uint32_t wq[8];
#pragma unroll
	for (int i = 0; i < 8; ++i) wq[i] = g32[i];
	float weight_norm = 0;
	for (int i = 0; i < S; ++i) {
		const int wv = (int)((wq[i >> 2] >> (8 * (i & 3))) & 255u);
		if (wv > 0) weight_norm += wv;
	}
	// hypotheses 3 and 4 are the same plane (strong_update_px): the second one is not evaluated
	const float hyp_depth[5] = { depth_rand, depth_now, depth_rand, depth_now, depth_pert };
	const f4 hyp_normal[5] = { plane_now, n_rand, n_rand, n_pert, plane_now };
	const float depth_entry = depth_now;
	const f4 plane_entry = plane_now;
	(void)depth_entry; (void)plane_entry;
	// A hypothesis is adopted iff its depth is in range and its weighted cost is below the running best (strict).
	// Two exact short cuts (the cost itself is only kept when adopted): (i) out of range -> not evaluated; (ii) the
	// weighted sum only grows — every term is a weight > 0 times a cost in [0, 2], IEEE addition and division are
	// monotone — so once the partial sum / weight_norm is not below cost_now the final one cannot be: the remaining
	// views are not evaluated.  Random hypotheses are rejected after one or two views instead of all selected ones.
	if (LANE_WALK) {
		// Round 4: every lane walks its OWN (hypothesis, view) sequence — one evaluation per trip of the loop below for
		// every lane that still has one — instead of the wave stepping through hypotheses and views together (where a
		// lane waits while any neighbour evaluates a view it did not select or a hypothesis it has already rejected:
		// lane utilisation 0.47).  Same evaluations per pixel in the same order, hence the same bits; the view index is
		// a per-lane value (ncc_old_lane).
		uint32_t sel = 0;     // views with a weight > 0
		for (int j = 0; j < S; ++j)
			if (((wq[j >> 2] >> (8 * (j & 3))) & 255u) > 0) sel |= 1u << j;
		int hyp = 0;
		bool busy = false;
		f4 plane = plane_now;
		float db = 0.0f, tc = 0.0f;
		uint32_t todo = 0;    // views of the current hypothesis not yet evaluated
		for (;;) {
			while (!busy && hyp < 5) {
				plane = hyp_normal[hyp];
				plane.w = distance_to_origin(rc, px, py, hyp_depth[hyp], plane);
				db = depth_from_plane(rc, plane, px, py);
				++hyp;
				if (!(db >= P.depth_min && db <= P.depth_max)) continue;
				if (!(weight_norm > 0.0f)) continue;      // no selected view: 0 / 0 = NaN, never below cost_now
				tc = 0.0f;
				todo = sel;
				busy = true;
			}
			if (!busy) break;
			const int j = dvp_ctz(todo);
			todo &= todo - 1;
			uint32_t q = wq[0];
#pragma unroll
			for (int k = 1; k < 8; ++k) q = (j >> 2) == k ? wq[k] : q;
			const int wv = (int)((q >> (8 * (j & 3))) & 255u);
			tc += wv * ncc_old_lane<SMP>(d, c, px, py, j + 1, plane);
			if (nevals) *nevals += 1;
			const bool alive = tc / weight_norm < cost_now;
			if (!alive) busy = false;
			else if (todo == 0) {      // the complete sum is below the running best
				depth_now = db;
				plane_now = plane;
				cost_now = tc / weight_norm;
				busy = false;
			}
		}
	} else
	for (int i = 0; i < 5; ++i) {
		f4 plane = hyp_normal[i];
		plane.w = distance_to_origin(rc, px, py, hyp_depth[i], plane);
		const float db = depth_from_plane(rc, plane, px, py);
		if (!(db >= P.depth_min && db <= P.depth_max)) continue;
		float tc = 0.0f;
		bool alive = weight_norm > 0.0f;     // no selected view: 0 / 0 = NaN, never below cost_now
		for (int j = 0; j < S && alive; ++j) {
			const int wv = (int)((wq[j >> 2] >> (8 * (j & 3))) & 255u);
			if (wv > 0) {
				tc += wv * ncc_old<SMP>(d, c, px, py, j + 1, plane);
				if (nevals) *nevals += 1;
				alive = tc / weight_norm < cost_now;
			}
		}
		if (alive) {      // == (tc / weight_norm < cost_now) of the complete sum
			depth_now = db;
			plane_now = plane;
			cost_now = tc / weight_norm;
		}
	}
	if (P.state == DVP_REFINE_INIT) {
		if (cost_now < costs_center - 0.1) {   // double comparison (APD.cu:2728)
			costs_center = cost_now;
			d.planes[center] = plane_now;
		}
	} else {
		costs_center = cost_now;
		d.planes[center] = plane_now;
	}
	d.costs[center] = costs_center;
}

// GetDepthandNormal (APD.cu:3167-3182)
DVP_HD void get_depth_normal_px(const Dev& d, int px, int py) {
	const int center = py * d.width + px;
	f4 pl = d.planes[center];
	pl.w = depth_from_plane(d.cameras[0], pl, px, py);
	d.planes[center] = normal_cam_to_world(d.cameras[0], pl);
}

// CheckerboardFilterStrong (APD.cu:3184-3294): median of the STRONG depths among self + 20 fixed
// opposite-colour offsets.
DVP_HD void filter_strong_px(const Dev& d, int px, int py) {
	const int W = d.width, H = d.height;
	const int center = py * W + px;
	if (d.costs[center] < 0.001f) return;
	float filter[21];
	int n = 0;
	filter[n++] = d.planes[center].w;
	// (dx, dy) in the reference's push order (APD.cu:3222-3284)
	const int ox[20] = { 0, 0, 0, 0, 0, 0, -1, -3, -5, 1, 3, 5, 2, 2, -2, -2, -1, 1, -1, 1 };
	const int oy[20] = { -1, -3, -5, 1, 3, 5, 0, 0, 0, 0, 0, 0, -1, 1, -1, 1, -2, -2, 2, 2 };
	for (int t = 0; t < 20; ++t) {
		const int x = px + ox[t], y = py + oy[t];
		if (x < 0 || y < 0 || x >= W || y >= H) continue;
		if (oy[t] == -2 && py <= 2) continue;   // the (+-1,-2) taps are guarded by p.y > 2 (APD.cu:3271,3275)
		const int q = x + y * W;
		if (d.weak_info[q] == DVP_STRONG) filter[n++] = d.planes[q].w;
	}
	sort_small(filter, n);
	const int m = n / 2;
	d.planes[center].w = (n % 2 == 0) ? (filter[m - 1] + filter[m]) / 2 : filter[m];
}

}  // namespace dvp
#endif
