// dvp_probe.inc — the DVP_PROBE micro-benchmark: its kernels, then its host entry dvp_probe.  Included by dvp_engine.hip,
// under #ifdef DVP_PROBE, after dvp_kernels.hpp and dvp_ctx.hpp.
// ---- mapping probe (experiment, not part of the product): K evaluations x S views per pixel with the planes of pixels
// `stride` apart, (A) lane = pixel like the NCC kernels, (B) lane = (pixel, view): 64 / S x-adjacent pixels per wave, the
// patch table of a pixel shared by its S lanes in LDS.
#ifndef DVP_PROBE_LB
#define DVP_PROBE_LB 2
#endif
extern "C" __global__ void __launch_bounds__(256, 2) dvp_probe_a(const Dev d, const LaunchArgs a, float* out, int K, int stride) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int px, py;
	if (!block_to_pixel(blockIdx.x, lane, wave, a.tiles_x, a.tiles, a.rows, 0, 0, d.width, d.height, &px, &py)) return;
	const int center = px + py * d.width;
	const int S = d.num_images - 1, L = d.width * d.height;
	PatchCtx c;
	__shared__ f2 lds_tab[kTaps * kTaps * 256];
	int radius, inc;
	patch_geometry(d, center, &radius, &inc);
	build_patch_ctx(d, px, py, radius, inc, 0, PatchTab{&lds_tab[threadIdx.x], 256}, &c);
	float acc = 0.0f;
	for (int k = 0; k < K; ++k) {
		int q = center + (k - K / 2) * stride;
		q = q < 0 ? 0 : (q >= L ? L - 1 : q);
		const f4 pl = d.planes[q];
		for (int v = 0; v < S; ++v) acc += ncc_old<0>(d, c, px, py, v + 1, pl);
	}
	out[center] = acc;
}
extern "C" __global__ void __launch_bounds__(256, DVP_PROBE_LB) dvp_probe_b(const Dev d, float* out, int K, int stride) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int S = d.num_images - 1, L = d.width * d.height;
	const int P = 64 / S;                                // pixels per wave
	const int waves_x = (d.width + P - 1) / P;
	const int gw = blockIdx.x * 4 + wave;
	const int py = gw / waves_x, x0 = (gw - py * waves_x) * P;
	if (py >= d.height) return;
	__shared__ f2 tab[4][9 * 36];                         // [wave][pixel][tap] (P <= 9... here P * 36 <= 324 for S >= 7)
	__shared__ float caa[4][9 * 36];
	__shared__ float sums[4][9][3];
	const int v = lane / P, pi = lane - v * P;           // lanes of one view are contiguous
	const int px = x0 + pi;
	const bool active = v < S && px < d.width;
	const int radius = d.params.strong_radius, inc = d.params.strong_increment;
	// table: entry e = pixel * 36 + tap, built by whichever lane
	for (int e = lane; e < P * 36; e += 64) {
		const int pe = e / 36, t = e - pe * 36, ty = t / 6, tx = t - ty * 6;
		const int qx = x0 + pe < d.width ? x0 + pe : d.width - 1;
		const float cpix = img_texel(d.images, d.org, d.pitch, d.width, d.height, qx, py);
		const float av = img_texel(d.images, d.org, d.pitch, d.width, d.height, qx - radius + tx * inc, py - radius + ty * inc);
		const float w = bilateral_weight((float)(-radius + tx * inc), (float)(-radius + ty * inc), av, cpix, d.params.sigma_spatial, d.params.sigma_color, 0);
		tab[wave][e] = mk2(w, w * av);
		caa[wave][e] = w * av * av;
	}
	__builtin_amdgcn_wave_barrier();
	if (lane < P) {
		float sr = 0.0f, srr = 0.0f, ws = 0.0f;
		for (int ty = 0; ty < 6; ++ty) {
			float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
			for (int tx = 0; tx < 6; ++tx) { const f2 t = tab[wave][lane * 36 + ty * 6 + tx]; a0 += t.y; a1 += caa[wave][lane * 36 + ty * 6 + tx]; a2 += t.x; }
			sr += a0; srr += a1; ws += a2;
		}
		sums[wave][lane][0] = sr; sums[wave][lane][1] = srr; sums[wave][lane][2] = ws;
	}
	__builtin_amdgcn_wave_barrier();
	if (!active) return;
	PatchCtx c;
	c.tab = PatchTab{&tab[wave][pi * 36], 1};
	c.sum_ref = sums[wave][pi][0]; c.sum_ref_ref = sums[wave][pi][1]; c.wsum = sums[wave][pi][2];
	c.radius = radius; c.inc = inc; c.fast = 1;
	const ViewConst vc = d.views[v + 1];                  // per-lane record (vector loads)
	const unsigned plane_off = (unsigned)((size_t)(v + 1) * d.plane_stride * 2 * sizeof(float));
	const int center = px + py * d.width;
	float acc = 0.0f;
	for (int k = 0; k < K; ++k) {
		int q = center + (k - K / 2) * stride;
		q = q < 0 ? 0 : (q >= L ? L - 1 : q);
		const f4 pl = d.planes[q];
		float H[9];
		homography(vc, pl, H);
		const f2 pt = apply_homography(H, px, py);
		if (pt.x >= vc.fw || pt.x < 0.0f || pt.y >= vc.fh || pt.y < 0.0f) { acc += 2.0f; continue; }
		acc += ncc_patch_fast<0>(d, c, H, d.images, px, py, plane_off);
	}
	atomicAdd(&out[center], acc);
}
// ---- round 6: the SWEEP-shaped probe (VERDICT r05 #1).  Work per pixel = DepthToWeak's: the 61 disparity slots around the
// pixel's own plane + the current depth, against the views of `vmask`.  (C) lane = pixel, slots in a loop — the mapping of
// dvp_sweep_eval; (D) wave = ONE pixel, lane = slot: the patch table is wave-uniform (288 B, read by LDS broadcast), a tap's 62
// gathers walk one epipolar segment.  Both sum a pixel's costs views-inside-slots in the same order: identical bits.
__device__ __forceinline__ float probe_slot_plane(const DvpCamera& rc, const f4 origin, float base_line, float disp, int k, int px, int py, const DvpParams& P, bool* in_range) {
	float p_depth = origin.w;
	*in_range = true;
	if (k < 61) {
		p_depth = rc.K[0] * base_line / (disp + (k - 30));
		if (p_depth < P.depth_min || p_depth > P.depth_max) *in_range = false;
	}
	return distance_to_origin(rc, px, py, p_depth, origin);
}
extern "C" __global__ void __launch_bounds__(256, 2) dvp_probe_c(const Dev d, const LaunchArgs a, float* out, unsigned vmask) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int px, py;
	if (!block_to_pixel(blockIdx.x, lane, wave, a.tiles_x, a.tiles, a.rows, 0, 0, d.width, d.height, &px, &py)) return;
	const int center = px + py * d.width;
	const int S = d.num_images - 1;
	PatchCtx c;
	__shared__ f2 lds_tab[kTaps * kTaps * 256];
	int radius, inc;
	patch_geometry(d, center, &radius, &inc);
	build_patch_ctx(d, px, py, radius, inc, 0, PatchTab{&lds_tab[threadIdx.x], 256}, &c);
	const DvpCamera rc = load_camera(d, 0);
	const f4 origin = normal_world_to_cam(rc, d.planes[center]);
	const float base_line = 0.4f, disp = rc.K[0] * base_line / origin.w;
	float acc = 0.0f;
	for (int k = 0; k < 62; ++k) {
		bool ok;
		f4 pl = origin;
		pl.w = probe_slot_plane(rc, origin, base_line, disp, k, px, py, d.params, &ok);
		float t = 0.0f;
		if (ok) for (int v = 0; v < S; ++v) if ((vmask >> v) & 1) t += ncc_old<0>(d, c, px, py, v + 1, pl);
		acc += t;
	}
	out[center] = acc;
}
#ifndef DVP_PROBE_NPX
#define DVP_PROBE_NPX 16
#endif
extern "C" __global__ void __launch_bounds__(64, DVP_PROBE_LB) dvp_probe_d(const Dev d, float* out, unsigned vmask) {
	const int lane = threadIdx.x;
	const int S = d.num_images - 1;
	__shared__ f2 ctab[kTaps * kTaps];
	__shared__ float caa[kTaps * kTaps];
	__shared__ float tot[64];
	// block -> run of DVP_PROBE_NPX pixels of one row: XCD b % 8 owns a 64-pixel column of a strip of 8, four runs per row, rows top to bottom
	const int runs = 64 / DVP_PROBE_NPX;
	const int tiles_x = (d.width + 63) / 64;
	const int per_strip = 8 * d.height * runs;
	const int st = (int)blockIdx.x / per_strip, rem = (int)blockIdx.x - st * per_strip;
	const int w_last = tiles_x - st * 8 >= 8 ? 8 : tiles_x - st * 8;
	const int col = rem % w_last, k2 = rem / w_last;
	const int py = k2 / runs, x0 = (st * 8 + col) * 64 + (k2 - py * runs) * DVP_PROBE_NPX;
	if (py >= d.height) return;
	const DvpCamera rc = load_camera(d, 0);
	for (int i = 0; i < DVP_PROBE_NPX; ++i) {
		const int px = x0 + i;
		if (px >= d.width) break;
		const int center = px + py * d.width;
		int radius, inc;
		patch_geometry(d, center, &radius, &inc);
		PatchCtx c;
		c.radius = radius; c.inc = inc; c.fast = 1;
		c.tab = PatchTab{ctab, 1};
		if (lane < kTaps * kTaps) {
			const int ty = lane / kTaps, tx = lane - ty * kTaps;
			const float cpix = img_texel(d.images, d.org, d.pitch, d.width, d.height, px, py);
			const float av = img_texel(d.images, d.org, d.pitch, d.width, d.height, px - radius + tx * inc, py - radius + ty * inc);
			const float w = bilateral_weight((float)(-radius + tx * inc), (float)(-radius + ty * inc), av, cpix, d.params.sigma_spatial, d.params.sigma_color, 0);
			const float wa = w * av;
			ctab[lane] = mk2(w, wa);
			caa[lane] = wa * av;
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		{
			float sr = 0.0f, srr = 0.0f, ws = 0.0f;
			for (int ty = 0; ty < kTaps; ++ty) {
				float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
				for (int tx = 0; tx < kTaps; ++tx) { const f2 t = ctab[ty * kTaps + tx]; a0 += t.y; a1 += caa[ty * kTaps + tx]; a2 += t.x; }
				sr += a0; srr += a1; ws += a2;
			}
			c.sum_ref = sr; c.sum_ref_ref = srr; c.wsum = ws;
		}
		f4 origin = normal_world_to_cam(rc, d.planes[center]);
		origin.x = uniform_f(origin.x); origin.y = uniform_f(origin.y); origin.z = uniform_f(origin.z); origin.w = uniform_f(origin.w);
		const float base_line = 0.4f, disp = rc.K[0] * base_line / origin.w;
		bool ok;
		f4 pl = origin;
		pl.w = probe_slot_plane(rc, origin, base_line, disp, lane, px, py, d.params, &ok);
		float t = 0.0f;
		if (lane < 62 && ok) for (int v = 0; v < S; ++v) if ((vmask >> v) & 1) t += ncc_old<0>(d, c, px, py, v + 1, pl);
		tot[lane] = t;
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		if (lane == 0) {
			float acc = 0.0f;
			for (int k = 0; k < 62; ++k) acc += tot[k];
			out[center] = acc;
		}
		__builtin_amdgcn_wave_barrier();
	}
}

extern "C" int dvp_probe(dvp_ctx* c, int mode, int K, int stride, int repeat, float* mean_ms, float* checksum) {
	if (set_device(c)) return 1;
	const LaunchGeom g = make_geom(c->W, c->H, false);
	LaunchArgs a;
	a.tiles_x = g.tiles_x; a.tiles = g.tiles; a.rows = g.rows; a.half = 0; a.colour = 0; a.iter = 0;
	const int S = c->NI - 1, P = 64 / S;
	const int waves = ((c->W + P - 1) / P) * c->H;
	EventPairGuard ev;
	HIP_TRY(c, hipEventCreate(&ev.a));
	HIP_TRY(c, hipEventCreate(&ev.b));
	for (int i = 0; i <= repeat; ++i) {
		if (i == 1) HIP_TRY(c, hipEventRecord(ev.a, c->stream));
		HIP_TRY(c, hipMemsetAsync(c->scratch_out, 0, c->L * 4, c->stream));
		if (mode == 0) hipLaunchKernelGGL(dvp_probe_a, dim3(g.grid()), dim3(256), 0, c->stream, c->d, a, c->scratch_out, K, stride);
		else if (mode == 1) hipLaunchKernelGGL(dvp_probe_b, dim3((waves + 3) / 4), dim3(256), 0, c->stream, c->d, c->scratch_out, K, stride);
		else if (mode == 2) hipLaunchKernelGGL(dvp_probe_c, dim3(g.grid()), dim3(256), 0, c->stream, c->d, a, c->scratch_out, (unsigned)K);   // K = view mask
		else hipLaunchKernelGGL(dvp_probe_d, dim3((unsigned)(g.tiles_x * c->H * (64 / DVP_PROBE_NPX))), dim3(64), 0, c->stream, c->d, c->scratch_out, (unsigned)K);
	}
	HIP_TRY(c, hipEventRecord(ev.b, c->stream));
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	float ms = 0.0f;
	HIP_TRY(c, hipEventElapsedTime(&ms, ev.a, ev.b));
	*mean_ms = ms / repeat;
	std::vector<float> h(c->L);
	HIP_TRY(c, hipMemcpy(h.data(), c->scratch_out, c->L * 4, hipMemcpyDeviceToHost));
	double sum = 0;
	for (float v : h) sum += v;
	*checksum = (float)(sum / (double)c->L);
	return 0;
}
