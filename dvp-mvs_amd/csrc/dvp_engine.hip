// dvp_engine.hip — the gfx950 PatchMatch engine: the C ABI of include/dvp_mvs.h and the launch functions.
//
// Replaces APD::CudaSpaceInitialization / SetDataPassHelperInCuda / RunPatchMatch
// (/root/reference/APD.cpp:1497-1613, 1670-1704; APD.cu:4406-4532).  One context owns one HIP
// stream and every device buffer of one reference view; launches are queued back to back on that
// stream (the reference calls cudaDeviceSynchronize after each of its 16+5*iters launches).
//
// This file is the C ABI and the launch functions.  It includes
//   dvp_kernels.hpp   LaunchArgs / ListArgs, the launch-bound defaults and every __global__ entry point
//   dvp_ctx.hpp       struct dvp_ctx, HIP_TRY and the context's arena (dalloc, dfree, alloc_group_or_fall_back)
//   dvp_probe.inc     the DVP_PROBE micro-benchmark, kernels and host entry (experiment builds only)
#include "dvp_kernels.hpp"
#include "dvp_ctx.hpp"
#ifdef DVP_PROBE
#include "dvp_probe.inc"
#endif
#include "dvp_pyramid_run.h"
#include <cstring>
#include <thread>
#include <chrono>
#include <algorithm>
#include <cmath>

extern "C" {

int dvp_ctx_create(int device, int width, int height, int num_images, dvp_ctx** out) {
	if (!out) return 1;
	*out = nullptr;
	if (width <= 0 || height <= 0 || num_images < 2 || num_images > DVP_MAX_IMAGES || width > 32767 || height > 32767) {
		g_create_error = "dvp_ctx_create: bad dimensions (2 <= num_images <= 32, sizes <= 32767: short2 pixel coordinates)";
		return 1;
	}
	{   // the samplers address a row-pair plane with 32-bit byte offsets
		const unsigned long long pitch = ((unsigned long long)width + 2 * kImgPad + 63) / 64 * 64;
		if (pitch * ((unsigned long long)height + 2 * kImgPad) * 8ull >= (1ull << 32)) {
			g_create_error = "dvp_ctx_create: image too large (a padded row-pair plane must stay below 4 GiB)";
			return 1;
		}
	}
	dvp_ctx* c = new dvp_ctx();
	c->device = device; c->W = width; c->H = height; c->NI = num_images;
	c->sw = read_form_switches();
	bump_reuse_epoch(c);
	c->pitch = (width + 2 * kImgPad + 63) / 64 * 64;
	c->L = (size_t)width * height;
	auto fail = [&](int) { g_create_error = c->error; dvp_ctx_destroy(c); return 1; };
	if (set_device(c)) return fail(0);
	if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { c->error = "hipStreamCreate failed"; return fail(0); }
	if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->side_fork, hipEventDisableTiming) != hipSuccess ||
	    hipEventCreateWithFlags(&c->side_join, hipEventDisableTiming) != hipSuccess) { c->error = "hipStreamCreate failed"; return fail(0); }
	const size_t L = c->L, S = (size_t)num_images - 1, plane = (size_t)c->pitch * (height + 2 * kImgPad);
	int r = 0;
	r |= dalloc(c, &c->images, plane * num_images * 2);
	r |= dalloc(c, &c->images8, (size_t)img8_tiles_x(width) * img8_tiles_y(height) * 128 * num_images);
	r |= dalloc(c, &c->images8_flag, (size_t)1);
	r |= dalloc(c, &c->image_stage, plane * num_images);
	r |= dalloc(c, &c->cameras, (size_t)num_images);
	r |= dalloc(c, &c->views, (size_t)num_images);
	r |= dalloc(c, &c->planes, L);
	r |= dalloc(c, &c->planes_snap, L);
	r |= dalloc(c, &c->search_pos, L * 16);
	r |= dalloc(c, &c->fit_planes, L);                     // cudaMemset 0, APD.cpp:1571
	r |= dalloc(c, &c->costs, L);
	r |= dalloc(c, &c->costs_snap, L);
	r |= dalloc(c, &c->selected_views, L + (size_t)width); // + one zeroed row (APD.cu:2473)
	r |= dalloc(c, &c->view_weight, L * 32);
	r |= dalloc(c, &c->weak_info, L);
	r |= dalloc(c, &c->weak_reliable, L);
	r |= dalloc(c, &c->weak_nearest_strong, L);
	r |= dalloc(c, &c->neighbours_map, L);
	r |= dalloc(c, &c->candidate, L * S * 8);
	r |= dalloc(c, &c->edge, L);
	r |= dalloc(c, &c->edge_bits, edge_bits_words(width, height));
	r |= dalloc(c, &c->strong_bits, edge_bits_words(width, height));
	r |= dalloc(c, &c->strong_bits_t, edge_bits_words(width, height));
	r |= dalloc(c, &c->edge_sat, (size_t)(sat_cells(width) + 1) * (sat_cells(height) + 1));
	r |= dalloc(c, &c->edge_neigh, L * 8);
	r |= dalloc(c, &c->label, L);
	r |= dalloc(c, &c->radius, L);
	r |= dalloc(c, &c->eval_counter, (size_t)1);
	r |= dalloc(c, &c->scratch_out, L);
	if (r) return fail(0);
	// defaults: every pixel STRONG (APD.cpp:1196-1204), radius = strong_radius (APD.cpp:1649-1653)
	{
		std::vector<uint8_t> st(L, (uint8_t)DVP_STRONG);
		std::vector<int> rad(L, 5);
		std::vector<s2> m1(L * 8, mks2(-1, -1));
		if (hipMemcpyAsync(c->weak_info, st.data(), L, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
			hipMemcpyAsync(c->radius, rad.data(), L * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
			hipMemcpyAsync(c->edge_neigh, m1.data(), L * 8 * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
			hipMemcpyAsync(c->weak_nearest_strong, m1.data(), L * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
			hipStreamSynchronize(c->stream) != hipSuccess) { c->error = "default state upload failed"; return fail(0); }
	}
	std::memset(&c->d.params, 0, sizeof(DvpParams));
	c->d.params.num_images = num_images;
	c->d.params.strong_radius = 5; c->d.params.strong_increment = 2; c->d.params.weak_radius = 5; c->d.params.weak_increment = 5;
	c->d.params.rotate_time = 4;
	sync_dev_struct(c);
	*out = c;
	return 0;
}

int dvp_ctx_destroy(dvp_ctx* c) {
	if (!c) return 0;
	// teardown: errors are not actionable here
	(void)hipSetDevice(c->device);
	{   // maps another thread is still fetching (dvp_download_maps_finish)
		// The driver relies on this wait: it hands a context back (and may destroy it) while the view's background job has
		// not fetched the staged maps yet.  Bounded all the same: maps that were staged and are never fetched — an exception
		// between the two steps — count as abandoned after DVP_DOWNLOAD_WAIT_S (120) seconds; a fetch that is RUNNING is
		// always waited for.
		int limit_s = 120;
		if (const char* e = getenv("DVP_DOWNLOAD_WAIT_S")) limit_s = atoi(e);
		std::unique_lock<std::mutex> lk(c->dl_m);
		c->dl_cv.wait_for(lk, std::chrono::seconds(limit_s > 0 ? limit_s : 1), [c] { return !c->dl_busy; });
		c->dl_cv.wait(lk, [c] { return !c->dl_fetching; });
	}
	if (c->copy) { (void)hipStreamSynchronize(c->copy); (void)hipStreamDestroy(c->copy); }
	if (c->pv_copy) { (void)hipStreamSynchronize(c->pv_copy); (void)hipStreamDestroy(c->pv_copy); }
	{   // a dvp_edge_map_finish that is running on another thread
		std::unique_lock<std::mutex> lk(c->eg_m);
		c->eg_cv.wait(lk, [c] { return !c->eg_slot[0].fetching && !c->eg_slot[1].fetching; });
	}
	if (c->eg_copy) { (void)hipStreamSynchronize(c->eg_copy); (void)hipStreamDestroy(c->eg_copy); }
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	dvpedge::scratch_free(c->eg);
	dvpvc::scratch_free(c->vc);
	// (the other side stages' blocks — pv_enc, eg_slot[].map, pr — are released by `delete c` below)
	for (auto& sl : c->eg_slot) if (sl.done) (void)hipEventDestroy(sl.done);
	if (c->pv_total) (void)hipHostFree(c->pv_total);
	if (c->pv_done) (void)hipEventDestroy(c->pv_done);
	if (c->maps_host) (void)hipHostFree(c->maps_host);
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	for (auto& e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
	for (void* p : c->allocs) (void)hipFree(p);
	if (c->weak_totals_host) (void)hipHostFree(c->weak_totals_host);
	if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
	if (c->side_fork) (void)hipEventDestroy(c->side_fork);
	if (c->side_join) (void)hipEventDestroy(c->side_join);
	if (c->stream) (void)hipStreamDestroy(c->stream);
	delete c;
	return 0;
}

#ifndef DVP_BUILD_ID
#define DVP_BUILD_ID "unknown"
#endif
const char* dvp_build_id(void) { return DVP_BUILD_ID; }

// dvp_download_maps_finish may run on another thread than the one that drives the context: its error text stays with
// the calling thread instead of racing with the driver thread's writes to dvp_ctx::error
struct FinishError { const dvp_ctx* c = nullptr; std::string msg; };
static thread_local FinishError t_finish_error;
const char* dvp_last_error(const dvp_ctx* c) {
	if (c && t_finish_error.c == c && !t_finish_error.msg.empty()) return t_finish_error.msg.c_str();
	return c ? c->error.c_str() : g_create_error.c_str();
}

static int finish_planes(dvp_ctx* c, float* dst, float* pairs);
// `pairs` != nullptr: `dst` is the staging set and the row-pair planes are produced from it
static int upload_planes(dvp_ctx* c, float* dst, const float* const* src, int pitch_floats, hipMemcpyKind kind, float* pairs = nullptr) {
	if (set_device(c)) return 1;
	if (pitch_floats < c->W) { c->error = "pitch_floats < width"; return 1; }
	const size_t stride = (size_t)c->pitch * (c->H + 2 * kImgPad);
	for (int i = 0; i < c->NI; ++i) {
		if (!src[i]) { c->error = "null image pointer"; return 1; }
		HIP_TRY(c, hipMemcpy2DAsync(dst + (size_t)i * stride + (size_t)kImgPad * c->pitch + kImgPad, (size_t)c->pitch * 4, src[i],
		                            (size_t)pitch_floats * 4, (size_t)c->W * 4, (size_t)c->H, kind, c->stream));
	}
	return finish_planes(c, dst, pairs);
}
// the interiors of the planes at `dst` are queued on the stream: the border, and with `pairs` every other form of the images
static int finish_planes(dvp_ctx* c, float* dst, float* pairs) {
	const size_t stride = (size_t)c->pitch * (c->H + 2 * kImgPad);
	{   // border replication == clamp-to-edge addressing (APD.cpp:1511-1515)
		const long long cells = (long long)(2 * kImgPad * (c->W + 2 * kImgPad) + 2 * kImgPad * c->H) * c->NI;
		hipLaunchKernelGGL(dvp_pad_replicate, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, dst, c->W, c->H, c->pitch, stride, c->NI);
		HIP_TRY(c, hipGetLastError());
	}
	if (pairs) {
		const int PH = c->H + 2 * kImgPad;
		hipLaunchKernelGGL(dvp_interleave_rows, dim3((unsigned)((c->pitch + 255) / 256), (unsigned)PH, (unsigned)c->NI), dim3(256), 0, c->stream,
		                   dst, pairs, PH, c->pitch, stride, c->NI);
		HIP_TRY(c, hipGetLastError());
		// byte planes for 8-bit exact image sets (Dev::images8), binary16 planes for binary16-exact ones (Dev::images16)
		HIP_TRY(c, hipMemsetAsync(c->images8_flag, 0, sizeof(int), c->stream));
		const int t8x = img8_tiles_x(c->W), t8y = img8_tiles_y(c->H);
		const size_t n = (size_t)t8x * t8y * 64 * c->NI;
		hipLaunchKernelGGL(dvp_pairs_to_tiles, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, pairs, c->images8, c->W + 2 * kImgPad, PH, c->pitch, stride,
		                   t8x, t8y, c->NI, c->images8_flag);
		HIP_TRY(c, hipGetLastError());
		int inexact = 3;
		HIP_TRY(c, hipMemcpyAsync(&inexact, c->images8_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		const int fmt = image_format(c->sw, (unsigned)inexact);
		c->images8_ok = fmt == 1;
		c->images16_ok = fmt == 2;
		if (c->images16_ok) {
			if (ensure_images16(c)) { c->images16_ok = false; sync_dev_struct(c); return 1; }
			const int t16x = img16_tiles_x(c->W), t16y = img16_tiles_y(c->H);
			const size_t n16 = (size_t)t16x * t16y * (kT16E * kT16H) * c->NI;
			hipLaunchKernelGGL(dvp_pairs_to_tiles16, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream, pairs, c->images16, c->W + 2 * kImgPad, PH, c->pitch, stride,
			                   t16x, t16y, c->NI);
			HIP_TRY(c, hipGetLastError());
		}
		sync_dev_struct(c);
	}
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return 0;
}
int dvp_upload_images(dvp_ctx* c, const float* const* images, int pitch_floats) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (upload_planes(c, c->image_stage, images, pitch_floats, hipMemcpyHostToDevice, c->images)) return 1;
	c->have_images = true;
	return 0;
}
int dvp_upload_images_device(dvp_ctx* c, const float* const* images, int pitch_floats) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (upload_planes(c, c->image_stage, images, pitch_floats, hipMemcpyDeviceToDevice, c->images)) return 1;
	c->have_images = true;
	return 0;
}
// the same images made on the device from the store's bytes (dvp_pyramid.hip): only the interiors' origin differs
int dvp_upload_images_u8(dvp_ctx* c, const dvp_images* store, const int* ids, int pad_w, int pad_h) {
	if (!c) return 1;
	if (!store || !ids) { c->error = "dvp_upload_images_u8: the store and the ids are required"; return 1; }
	if (pad_w < 1 || pad_h < 1 || pad_w > 32767 || pad_h > 32767) { c->error = "dvp_upload_images_u8: bad canvas size (1 ... 32767)"; return 1; }
	if (dvppyr::store_device(store) != c->device) { c->error = "dvp_upload_images_u8: the store is on another device than the context"; return 1; }
	dvppyr::Sources src;
	std::string message;
	if (dvppyr::store_sources(store, ids, c->NI, &src, &message)) { c->error = "dvp_upload_images_u8: " + message; return 1; }
	if (src.v[0].sw != pad_w || src.v[0].sh != pad_h) { c->error = "dvp_upload_images_u8: the reference image (ids[0]) must have the canvas size"; return 1; }
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	const size_t stride = (size_t)c->pitch * (c->H + 2 * kImgPad);
	if (dvppyr::launch_levels(c->stream, src, c->NI, pad_w, pad_h, c->W, c->H, c->image_stage + (size_t)kImgPad * c->pitch + kImgPad, c->pitch, stride)) {
		c->error = "dvp_upload_images_u8: launch failed";
		return 1;
	}
	if (finish_planes(c, c->image_stage, c->images)) return 1;
	c->have_images = true;
	return 0;
}
int dvp_download_image(dvp_ctx* c, int index, float* out, int pitch_floats) {
	if (!c) return 1;
	if (!out || index < 0 || index >= c->NI || pitch_floats < c->W) { c->error = "dvp_download_image: bad arguments (0 <= index < num_images, pitch_floats >= width)"; return 1; }
	if (!c->have_images) { c->error = "dvp_download_image: no images in the context yet (dvp_upload_images)"; return 1; }
	if (set_device(c)) return 1;
	const size_t stride = (size_t)c->pitch * (c->H + 2 * kImgPad);
	HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)pitch_floats * 4, c->image_stage + (size_t)index * stride + (size_t)kImgPad * c->pitch + kImgPad, (size_t)c->pitch * 4,
	                            (size_t)c->W * 4, (size_t)c->H, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return 0;
}
static int ensure_depths(dvp_ctx* c) {
	if (!c->depths) {
		if (dalloc(c, &c->depths, (size_t)c->pitch * (c->H + 2 * kImgPad) * c->NI)) return 1;
		sync_dev_struct(c);
	}
	c->have_depths = true;
	return 0;
}
int dvp_upload_depths(dvp_ctx* c, const float* const* depths, int pitch_floats) {
	if (set_device(c) || ensure_depths(c)) return 1;
	return upload_planes(c, c->depths, depths, pitch_floats, hipMemcpyHostToDevice);
}
int dvp_upload_depths_device(dvp_ctx* c, const float* const* depths, int pitch_floats) {
	if (set_device(c) || ensure_depths(c)) return 1;
	return upload_planes(c, c->depths, depths, pitch_floats, hipMemcpyDeviceToDevice);
}

int dvp_upload_cameras(dvp_ctx* c, const DvpCamera* cams, int n) {
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	if (n != c->NI) { c->error = "dvp_upload_cameras: n != num_images"; return 1; }
	HIP_TRY(c, hipMemcpyAsync(c->cameras, cams, sizeof(DvpCamera) * n, hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(dvp_prepare_views, dim3(1), dim3(64), 0, c->stream, c->cameras, c->views, n);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->have_cameras = true;
	return 0;
}

// The FIRST_INIT plane prior from the Depth-Anything map and the sparse SfM points (dvp_prior.hip): the planes BuildPlanePrior
// (host/prior.cpp) computes, bit for bit, written by the device into the context's planes.
int dvp_plane_prior(dvp_ctx* c, const float* dep_raw, int dep_w, int dep_h, const float* xy, const float* xyz, int num_points, const DvpCamera* file_camera, int* status) {
	if (!c) return 1;
	if (!status || !file_camera || num_points < 0 || (num_points > 0 && (!xy || !xyz)) || dep_w < 0 || dep_h < 0 || ((long long)dep_w * dep_h > 0 && !dep_raw)) {
		c->error = "dvp_plane_prior: the status pointer, the camera, the points and the map are required";
		return 1;
	}
	if (!c->have_cameras) { c->error = "dvp_plane_prior: no cameras in the context yet (dvp_upload_cameras)"; return 1; }
	if (set_device(c)) return 1;
	const char* what = "";
	if (dvpprior::run(c->stream, c->pr, dep_raw, dep_w, dep_h, xy, xyz, num_points, file_camera, c->cameras, c->W, c->H, c->planes, status, &what)) { c->error = what; return 1; }
	if (*status == 0) {
		c->anchor_tab_valid = false;
		bump_reuse_epoch(c);
	}
	return 0;
}

int dvp_plane_prior_stage(dvp_ctx* c, int which, void* dst) {
	if (!c) return 1;
	if (!dst) { c->error = "dvp_plane_prior_stage: the destination is required"; return 1; }
	if (set_device(c)) return 1;
	const char* what = "";
	if (dvpprior::stage(c->stream, c->pr, which, dst, &what)) { c->error = what; return 1; }
	return 0;
}

int dvp_plane_prior_timings(dvp_ctx* c, double* ms, long long* counts) {
	if (!c) return 1;
	if (!c->pr.ran) { c->error = "dvp_plane_prior_timings: no dvp_plane_prior with status 0 has finished on this context"; return 1; }
	if (ms) for (int k = 0; k < 3; ++k) ms[k] = c->pr.ms[k];
	if (counts) { counts[0] = c->pr.triangles; counts[1] = c->pr.sweep_rows; }
	return 0;
}

static int ensure_weak_buffers(dvp_ctx* c, size_t weak_count) {
	const size_t need = weak_count ? weak_count : 1;
	if (need > c->weak_alloc) {
		// The host driver recycles one context over all views and passes (APD.cpp pool): grow geometrically and give the
		// superseded blocks back.
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		if (c->side) HIP_TRY(c, hipStreamSynchronize(c->side));
		dfree(c, &c->neighbours); dfree(c, &c->gn_points); dfree(c, &c->gn_count); dfree(c, &c->complex_); dfree(c, &c->label_boundary);
		const size_t cap = std::min<size_t>(c->L, std::max(need, c->weak_alloc + c->weak_alloc / 2));
		if (dalloc(c, &c->neighbours, cap * DVP_NEIGHBOUR_NUM, false)) return 1;
		if (dalloc(c, &c->gn_points, cap * kGnDirSlots, false) || dalloc(c, &c->gn_count, cap)) return 1;
		if (dalloc(c, &c->complex_, cap)) return 1;
		if (dalloc(c, &c->label_boundary, cap * 8, false)) return 1;
		c->weak_alloc = cap;
	}
	HIP_TRY(c, hipMemsetAsync(c->neighbours, 0xFF, need * DVP_NEIGHBOUR_NUM * sizeof(s2), c->stream));   // (-1,-1)
	HIP_TRY(c, hipMemsetAsync(c->label_boundary, 0xFF, need * 8 * sizeof(s2), c->stream));
	HIP_TRY(c, hipMemsetAsync(c->complex_, 0, need * 4, c->stream));
	return 0;
}

// weak_info (on the device) -> neighbours_map, the compacted WEAK lists, the per-WEAK buffers
static int rebuild_weak_lists(dvp_ctx* c) {
	const size_t L = c->L;
	// weak_info -> neighbours_map (running index of WEAK pixels, APD.cpp:1182-1193) and the compacted WEAK lists of the
	// list kernels (black, then red; rows the reference's half grid never reaches, APD.cu:4421-4424, are kept like in the
	// full-grid launch), all on the device: see dvp_weak_counts / dvp_scan3 / dvp_weak_fill.  List order = 64 x 64
	// super-tiles, 16 x 16 tiles inside them, rows inside those: the lanes of a wave are neighbours in both directions and
	// the ~8 consecutive workgroups of a super-tile share their anchors and the source lines those touch; stage_body_list
	// hands such runs to ONE XCD.  (16x16 vs 16x8 / 32x4 / row-major: 592.7 / 599 / 609 / 622 ms per REFINE pass, r01.)
	// Every list kernel is order-independent (a WEAK pixel only reads STRONG pixels' state).
	const int supers_x = (c->W + kWeakSuper - 1) / kWeakSuper, supers_y = (c->H + kWeakSuper - 1) / kWeakSuper;
	const int n_slots = supers_x * supers_y * 16, n_chunks = (int)((L + kWeakChunk - 1) / kWeakChunk);
	const int n_units = n_slots + n_chunks;
	if (!c->weak_counts) {
		if (dalloc(c, &c->weak_counts, (size_t)2 * n_slots + n_chunks + 4)) return 1;
		HIP_TRY(c, hipHostMalloc((void**)&c->weak_totals_host, 4 * sizeof(int)));
	}
	int* totals = c->weak_counts + 2 * (size_t)n_slots + n_chunks;
	hipLaunchKernelGGL(dvp_weak_counts, dim3((n_units + 3) / 4), dim3(256), 0, c->stream, c->weak_info, c->W, c->H, supers_x, n_slots, n_chunks, c->weak_counts);
	hipLaunchKernelGGL(dvp_scan3, dim3(3), dim3(1024), 0, c->stream, c->weak_counts, 0, n_slots, 2 * n_slots, 2 * n_slots + n_chunks, totals);
	HIP_TRY(c, hipMemcpyAsync(c->weak_totals_host, totals, 3 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	const int nb = c->weak_totals_host[0], nr = c->weak_totals_host[1], wc = c->weak_totals_host[2];
	if (nb + nr != wc) { c->error = "dvp_upload_state: WEAK list / map counts disagree"; return 1; }
	c->d.weak_count = wc;
	c->d.weak_black = nb;
	c->d.weak_red = nr;
	if ((size_t)wc > c->weak_list_alloc) {
		dfree(c, &c->weak_list);
		const size_t cap = std::min<size_t>(L, std::max<size_t>((size_t)wc, c->weak_list_alloc + c->weak_list_alloc / 2));
		if (dalloc(c, &c->weak_list, cap, false)) return 1;
		c->weak_list_alloc = cap;
	}
	if (wc > 0) {
		hipLaunchKernelGGL(dvp_weak_fill, dim3((n_units + 3) / 4), dim3(256), 0, c->stream, c->weak_info, c->W, c->H, supers_x, n_slots, n_chunks,
		                   c->weak_counts, totals, c->weak_list, c->neighbours_map);
		HIP_TRY(c, hipGetLastError());
	} else {
		HIP_TRY(c, hipMemsetAsync(c->neighbours_map, 0, L * 4, c->stream));
	}
	if (ensure_weak_buffers(c, (size_t)wc)) return 1;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	sync_dev_struct(c);
	return 0;
}

int dvp_upload_state(dvp_ctx* c, const float* planes, const uint32_t* views, const uint8_t* weak,
                     const uint8_t* edge, const int32_t* label, const int32_t* radius) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	const size_t L = c->L;
	if (planes) HIP_TRY(c, hipMemcpyAsync(c->planes, planes, L * 16, hipMemcpyHostToDevice, c->stream));
	if (views) HIP_TRY(c, hipMemcpyAsync(c->selected_views, views, L * 4, hipMemcpyHostToDevice, c->stream));
	if (edge) HIP_TRY(c, hipMemcpyAsync(c->edge, edge, L, hipMemcpyHostToDevice, c->stream));
	if (label) HIP_TRY(c, hipMemcpyAsync(c->label, label, L * 4, hipMemcpyHostToDevice, c->stream));
	if (radius) HIP_TRY(c, hipMemcpyAsync(c->radius, radius, L * 4, hipMemcpyHostToDevice, c->stream));
	if (weak) HIP_TRY(c, hipMemcpyAsync(c->weak_info, weak, L, hipMemcpyHostToDevice, c->stream));
	return rebuild_weak_lists(c);
}

// The per-pixel input state of a REFINE_INIT pass from the coarser level's result maps, up-sampled on the device
// (dvp_rescale_state): 25 bytes per COARSE pixel cross the bus instead of 25 per fine one, and the host neither rescales
// nor assembles planes.
int dvp_upload_state_rescaled(dvp_ctx* c, int src_w, int src_h, const float* depth, const float* normal_xyz, const uint32_t* views,
                              const uint8_t* weak, const int32_t* radius, int radius_fallback, const uint8_t* edge, const int32_t* label) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	if (src_w <= 0 || src_h <= 0 || !depth || !normal_xyz || !views) { c->error = "dvp_upload_state_rescaled: depth, normal and selected_views are required"; return 1; }
	const size_t L = c->L, n = (size_t)src_w * src_h;
	const size_t off_normal = n * 4, off_views = off_normal + n * 12, off_radius = off_views + n * 4, off_weak = off_radius + n * 4, bytes = off_weak + n;
	if (bytes > c->coarse_alloc) {
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		dfree(c, &c->coarse);
		if (dalloc(c, &c->coarse, bytes, false)) return 1;
		c->coarse_alloc = bytes;
	}
	HIP_TRY(c, hipMemcpyAsync(c->coarse, depth, n * 4, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->coarse + off_normal, normal_xyz, n * 12, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->coarse + off_views, views, n * 4, hipMemcpyHostToDevice, c->stream));
	if (radius) HIP_TRY(c, hipMemcpyAsync(c->coarse + off_radius, radius, n * 4, hipMemcpyHostToDevice, c->stream));
	if (weak) HIP_TRY(c, hipMemcpyAsync(c->coarse + off_weak, weak, n, hipMemcpyHostToDevice, c->stream));
	if (edge) HIP_TRY(c, hipMemcpyAsync(c->edge, edge, L, hipMemcpyHostToDevice, c->stream));
	if (label) HIP_TRY(c, hipMemcpyAsync(c->label, label, L * 4, hipMemcpyHostToDevice, c->stream));
	RescaleArgs a;
	a.W = c->W; a.H = c->H; a.sw = src_w; a.sh = src_h;
	a.scale_x = c->W / static_cast<float>(src_w);
	a.scale_y = c->H / static_cast<float>(src_h);
	a.depth = reinterpret_cast<const float*>(c->coarse); a.normal = reinterpret_cast<const float*>(c->coarse + off_normal);
	a.views = reinterpret_cast<const uint32_t*>(c->coarse + off_views);
	a.radius = radius ? reinterpret_cast<const int*>(c->coarse + off_radius) : nullptr;
	a.weak = weak ? c->coarse + off_weak : nullptr;
	a.planes = c->planes; a.out_views = c->selected_views; a.out_weak = c->weak_info; a.out_radius = c->radius;
	a.radius_fallback = radius_fallback;
	hipLaunchKernelGGL(dvp_rescale_state, dim3((unsigned)((c->W + 255) / 256), (unsigned)c->H), dim3(256), 0, c->stream, a);
	HIP_TRY(c, hipGetLastError());
	return rebuild_weak_lists(c);
}

int dvp_reset_state(dvp_ctx* c) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	const size_t L = c->L;
	HIP_TRY(c, hipMemsetAsync(c->planes, 0, L * 16, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->fit_planes, 0, L * 16, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->costs, 0, L * 4, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->selected_views, 0, (L + c->W) * 4, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->view_weight, 0, L * 32, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->weak_info, DVP_STRONG, L, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->edge, 0, L, c->stream));        // a recycled context must not see the previous view's priors
	HIP_TRY(c, hipMemsetAsync(c->label, 0, L * 4, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->neighbours_map, 0, L * 4, c->stream));
	HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)c->radius, c->d.params.strong_radius, L, c->stream));
	c->d.weak_count = 0;
	c->d.weak_black = c->d.weak_red = 0;
	if (ensure_weak_buffers(c, 0)) return 1;
	sync_dev_struct(c);
	return 0;
}

// Device-side snapshot of the per-pixel INPUT state of a pass (what dvp_upload_state delivers:
// planes, selected_views, weak_info, radius; the WEAK-pixel list and neighbours_map derived from
// weak_info stay valid because the same weak map comes back) and its restore, which also returns the
// pass-internal buffers to their freshly-uploaded content.  Lets a caller run the same pass again
// from identical inputs (bench steps, A/B checks) without a host round trip.
int dvp_image_format(const dvp_ctx* c) { return !c ? 0 : (c->images8_ok ? 1 : (c->images16_ok ? 2 : 0)); }
int dvp_strong_update_form(const dvp_ctx* c) {
	if (!c) return 0;
	const StrongForm f = strong_form(c->sw, c->NI - 1, c->split_fits, false, 0);
	return f.kernel == STRONG_SPLIT ? f.decide : 0;
}
int dvp_save_state(dvp_ctx* c) {
	if (set_device(c)) return 1;
	const size_t L = c->L;
	if (!c->saved_planes) {
		if (dalloc(c, &c->saved_planes, L, false) || dalloc(c, &c->saved_views, L, false) ||
			dalloc(c, &c->saved_weak, L, false) || dalloc(c, &c->saved_radius, L, false)) return 1;
	}
	HIP_TRY(c, hipMemcpyAsync(c->saved_planes, c->planes, L * 16, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->saved_views, c->selected_views, L * 4, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->saved_weak, c->weak_info, L, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->saved_radius, c->radius, L * 4, hipMemcpyDeviceToDevice, c->stream));
	c->have_saved = true;
	return 0;
}
int dvp_restore_state(dvp_ctx* c) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	if (!c->have_saved) { c->error = "dvp_restore_state: no saved state"; return 1; }
	const size_t L = c->L;
	HIP_TRY(c, hipMemcpyAsync(c->planes, c->saved_planes, L * 16, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->selected_views, c->saved_views, L * 4, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->weak_info, c->saved_weak, L, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->radius, c->saved_radius, L * 4, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->fit_planes, 0, L * 16, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->costs, 0, L * 4, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->view_weight, 0, L * 32, c->stream));
	HIP_TRY(c, hipMemsetAsync(c->weak_reliable, 0, L, c->stream));
	if (ensure_weak_buffers(c, (size_t)c->d.weak_count)) return 1;
	return 0;
}

int dvp_set_params(dvp_ctx* c, const DvpParams* p) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	if (p->num_images != c->NI) { c->error = "dvp_set_params: params.num_images != context num_images"; return 1; }
	if (p->use_edge == 0) { c->error = "dvp_set_params: use_edge=false is rejected: the reference's legacy ACMH branch (APD.cu:2142-2460) adopts planes through positions[], which only the use_edge branch assigns (APD.cu:2036, 2084, 2133 vs 2559-2563) - it has no defined result to reproduce"; return 1; }
	if (p->weak_radius < 0 || p->weak_radius > 15) { c->error = "dvp_set_params: weak_radius out of range [0,15]"; return 1; }
	c->d.params = *p;
	set_neighbour_consts(&c->d);
	if (c->lut_radius != p->weak_radius) {
		std::vector<int> taps, start;
		make_sector_taps(p->weak_radius, &taps, &start);
		if (dalloc(c, &c->sector_taps, taps.size(), false) || dalloc(c, &c->sector_start, start.size(), false)) return 1;
		HIP_TRY(c, hipMemcpyAsync(c->sector_taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipMemcpyAsync(c->sector_start, start.data(), start.size() * 4, hipMemcpyHostToDevice, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		c->lut_radius = p->weak_radius;
	}
	sync_dev_struct(c);
	return 0;
}
int dvp_set_seed(dvp_ctx* c, uint64_t seed) { c->d.seed = seed; return 0; }
int dvp_set_sampler(dvp_ctx* c, int s) { c->d.sampler = s ? 1 : 0; bump_reuse_epoch(c); return 0; }
int dvp_set_profiling(dvp_ctx* c, int on) { c->profiling = on != 0; sync_dev_struct(c); return 0; }

// ---- optional buffers ---------------------------------------------------------------------------
// The buffers only one form of a launch site needs are allocated at the first launch that wants them, or ahead of it by
// dvp_ctx_reserve, off the critical path (a multi-GB hipMalloc inside a launch site took 0.5-1 s of a view on some boxes:
// profiles/r06_ab_notes.txt).  A group that does not fit is not an error: the site takes the form that does without — the same bits.

// The pass' table of anchor reference sides (dvp_weak_wave.hpp: build_anchor_record) — built at the first weak update after
// anything that can change the anchors (GenNeighbours, NeigbourUpdate), the offsets (GenEdgeInform), the images or the WEAK
// list; the iterations of a pass then share it.
// room in the anchor table for `wc` WEAK pixels (grown with half as much again on top: the views of a level differ in their WEAK
// counts, and every regrow is a device-wide free + a multi-GB allocation)
static int grow_anchor_table(dvp_ctx* c, size_t wc) {
	const size_t need = wc * (size_t)(c->NI - 1) * kAnchors;
	if (anchor_table_off(c) || need <= c->anchor_tab_alloc) return 0;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	dfree(c, &c->anchor_tab);
	c->anchor_tab_alloc = 0;
	c->anchor_tab_alloc = alloc_group_or_fall_back(c, { areq(&c->anchor_tab, (need + need / 2) * sizeof(AnchorRec)) }, nullptr, &c->anchor_tab_fits,
		"dvp: no room for the weak update's anchor table (%.1f GB); forming the reference side per item\n", (double)need * sizeof(AnchorRec) / 1e9,
		need * sizeof(AnchorRec)) / sizeof(AnchorRec);
	return 0;
}
static int ensure_anchor_table(dvp_ctx* c, int covered_rows) {
	if (anchor_table_off(c) || c->anchor_tab_valid) return 0;
	const int wc = c->d.weak_black + c->d.weak_red;
	if (grow_anchor_table(c, (size_t)wc)) return 1;
	if (anchor_table_off(c)) return 0;
	c->anchor_tab_valid = true;
	sync_dev_struct(c);
	ListArgs la;
	la.base = 0; la.count = wc; la.iter = 0; la.covered_rows = covered_rows;
	const long long n = (long long)wc * (c->NI - 1) * kAnchors;
	if (n > 0) {
		hipLaunchKernelGGL(dvp_weak_anchor_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d, la);
		HIP_TRY(c, hipGetLastError());
	}
	return 0;
}

// hand-over buffers of the phased weak update (624 + 32 S bytes per WEAK pixel: 1.6 GB at 6208x4128 with 7 % WEAK, S = 9)
static int grow_weak_phase_buffers(dvp_ctx* c, size_t wc) {
	if (!c->sw.weak_phased || !c->weak_phase_fits || wc <= c->weak_phase_alloc) return 0;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	dfree(c, &c->weak_rec); dfree(c, &c->weak_ctab); dfree(c, &c->weak_ev);
	c->weak_phase_alloc = 0;
	const size_t cap = std::min<size_t>(c->L, wc + wc / 2), S = (size_t)c->NI - 1;
	if (alloc_group_or_fall_back(c, { areq(&c->weak_rec, cap * sizeof(WeakRec)), areq(&c->weak_ctab, cap * kTaps * kTaps * sizeof(f2)), areq(&c->weak_ev, cap * 8 * S * sizeof(float)) },
			"DVP_TEST_WEAK_PHASE_ALLOC_FAIL", &c->weak_phase_fits, "dvp: no room for the phased weak update's hand-over buffers (%.2f GB); using the one-wave kernel\n", (double)cap * (sizeof(WeakRec) + 288 + 32 * S) / 1e9))
		c->weak_phase_alloc = cap;
	return 0;
}

// The plane cache's records: 17 x S floats + 17 keys + a header per pixel of the whole image (15.7 + 7.0 + 0.4 GB at 6208x4128,
// S = 9), in place of the half-size slot_costs (7.8 GB), which such a context never allocates.  A context that cannot have them
// keeps slot_costs and evaluates every distinct plane at every visit.
static void ensure_strong_reuse_buffers(dvp_ctx* c) {
	if (c->reuse_costs || !c->sw.strong_reuse || !c->reuse_fits || strong_form(c->sw, c->NI - 1, c->split_fits, false, 0).kernel != STRONG_SPLIT) return;
	const size_t L = c->L, vec = (size_t)kSlotCount * (c->NI - 1) * L * sizeof(float) + 64 /* load_slot_costs reads whole 16-byte pieces */;
	const size_t Lh = (size_t)((c->W + 1) / 2) * c->H;
	alloc_group_or_fall_back(c, { areq(&c->reuse_costs, vec), areq(&c->reuse_keys, L * kSlotCount * sizeof(PlaneKey)), areq(&c->reuse_hdr, L * sizeof(ReuseHdr), true),
			c->strong_rec ? AllocReq{} : areq(&c->strong_rec, (size_t)SR_FIELDS * Lh * sizeof(*c->strong_rec)) },
		"DVP_TEST_REUSE_ALLOC_FAIL", &c->reuse_fits, "dvp: no room for the strong update's plane cache (%.1f GB); every visit evaluates all its planes\n", (double)(vec + L * (kSlotCount * sizeof(PlaneKey) + sizeof(ReuseHdr))) / 1e9);
}
static void ensure_strong_split_buffers(dvp_ctx* c) {
	if (c->slot_costs || strong_form(c->sw, c->NI - 1, c->split_fits, false, 0).kernel != STRONG_SPLIT) return;
	if (!getenv("DVP_TEST_SPLIT_ALLOC_FAIL")) {
		ensure_strong_reuse_buffers(c);
		if (c->reuse_costs) return;   // the full-size records stand in for slot_costs
	}
	// 17 x S floats per pixel of one colour (7.8 GB at 6208x4128, S = 9): a part that cannot spare them runs the
	// monolithic kernel instead, which gives the same bits (test_strong_update_forms_equal_the_oracle)
	const size_t Lh = (size_t)((c->W + 1) / 2) * c->H;
	alloc_group_or_fall_back(c, { areq(&c->slot_costs, (size_t)kSlotCount * (c->NI - 1) * Lh * sizeof(*c->slot_costs) + 64 /* load_slot_costs reads whole 16-byte pieces */),
			areq(&c->strong_rec, (size_t)SR_FIELDS * Lh * sizeof(*c->strong_rec)) },
		"DVP_TEST_SPLIT_ALLOC_FAIL", &c->split_fits, "dvp: no room for the split strong update's cost buffer (%.1f GB); using the monolithic kernel\n", (double)kSlotCount * (c->NI - 1) * Lh * 4 / 1e9);
}
// 73 floats per (pixel, view) + 61 + 8 per pixel (67 GB at 6208x4128, S = 9); the cost records of the whole image, or of a band of
// rows when the context is told to keep them small (fresh device memory is 31-40 ms per GB on this part, tools/micro/alloc_time.hip:
// 2.3 s for a 25-Mpx view's 67 GB)
static void ensure_sweep_buffers(dvp_ctx* c) {
	if (c->sweep_cost || !c->sw.sweep_split || !c->sweep_fits) return;
	const size_t L = c->L;
	c->sweep_band_rows = sweep_band_rows(c->sw, c->W, c->H, c->NI - 1);
	const size_t band_px = c->sweep_band_rows > 0 ? (size_t)c->sweep_band_rows * c->W : L;
	alloc_group_or_fall_back(c, { areq(&c->sweep_rec, 2 * L * sizeof(f4)), areq(&c->sweep_pc, 61 * L * sizeof(float)), areq(&c->sweep_cost, sweep_cost_floats(band_px, c->NI - 1) * sizeof(float)) },
		"DVP_TEST_SWEEP_ALLOC_FAIL", &c->sweep_fits, "dvp: no room for the view-compacted DepthToWeak's cost buffer (%.1f GB); using the fused kernel\n", (double)(c->NI - 1) * kSweepFields * L * 4 / 1e9);
}
// The evaluation launches' per-view lists: 4 bytes per (pixel, view) of the image or of a band (0.9 GB at 6208x4128, S = 9; one
// buffer: a stage's lists are consumed before the next stage's are built, in stream order), the counts per (view, tile) and the
// lengths.  A context that cannot have them evaluates tile by tile.
static void ensure_sweep_list_buffers(dvp_ctx* c) {
	if (c->sweep_list || !c->sweep_cost || !c->sw.sweep_list || !c->sweep_list_fits) return;
	const size_t S = (size_t)c->NI - 1;
	const int band_rows = c->sweep_band_rows > 0 ? c->sweep_band_rows : c->H;
	c->sweep_list_cap = band_rows * c->W;
	c->sweep_list_tiles = ((c->W + 63) / 64) * ((band_rows + kSweepRows - 1) / kSweepRows);
	alloc_group_or_fall_back(c, { areq(&c->sweep_list, S * (size_t)c->sweep_list_cap * sizeof(uint32_t)), areq(&c->sweep_list_counts, (S * c->sweep_list_tiles + (S + 2) / 3 * 3) * sizeof(int)) },
		"DVP_TEST_SWEEP_LIST_ALLOC_FAIL", &c->sweep_list_fits, "dvp: no room for the sweep passes' (pixel, view) lists (%.2f GB); evaluating tile by tile\n", (double)S * c->sweep_list_cap * 4 / 1e9);
}

// ---- launches ---------------------------------------------------------------------------------
// Which kernels a launch site runs is decided by dvp_forms.hpp; the functions below issue them.
// `fused` (dvp_run_patchmatch only): DepthToWeak does LocalRefine too; GenEdgeInform leaves the visibility-prior
// candidates to dvp_run_patchmatch (side stream; not computed at all when the pass has no WEAK pixel: their only
// reader is the weak update's anchor_cost)

// the instantiation of kernel NAME for the context's sampler, and for the image format `fmt` of the set
#define DVP_PICK(NAME, SUF) (c->d.sampler ? NAME##_exact##SUF : NAME##SUF)
#define DVP_PICK_FMT(NAME, TAIL) (fmt == 1 ? DVP_PICK(NAME, _u8##TAIL) : (fmt == 2 ? DVP_PICK(NAME, _f16##TAIL) : DVP_PICK(NAME, TAIL)))

static LaunchArgs make_args(const LaunchGeom& g, int colour, int iter) {
	LaunchArgs a;
	a.tiles_x = g.tiles_x; a.tiles = g.tiles; a.rows = g.rows; a.half = g.half ? 1 : 0;
	a.colour = colour; a.iter = iter;
	return a;
}

// the visibility-prior candidates of `blocks` x 256 pixels of the image (a) or of the pixel list, with the state `d` sees
static void launch_gen_candidates(dvp_ctx* c, hipStream_t stream, const Dev& d, unsigned blocks, const LaunchArgs& a, const unsigned* list = nullptr, const unsigned* n_list = nullptr) {
	const bool all = gen_candidates_all_views(d);
	const dim3 grid(blocks, all ? (unsigned)((c->NI - 1 + kCandGroup - 1) / kCandGroup) : (unsigned)(c->NI - 1)), block(256);
	if (list) hipLaunchKernelGGL(all ? dvp_gen_candidates_views_list : dvp_gen_candidates_list, grid, block, 0, stream, d, list, n_list);
	else hipLaunchKernelGGL(all ? dvp_gen_candidates_views : dvp_gen_candidates, grid, block, 0, stream, d, a);
}

// pre-launch snapshot: the direction-4 samples of the strong update are same-colour pixels
// (APD.cu:2071-2074); every neighbour read of that kernel sees the state before the launch.
// Then the light sample-search launch.  Both are timed in their own bucket (DVP_ST_STRONG_PREP)
// so that stage_ms[DVP_ST_STRONG_UPDATE] is the update kernel alone.
static int launch_strong_prep(dvp_ctx* c, const LaunchGeom& g, const LaunchArgs& a) {
	EventPair prep;
	prep.stage = DVP_ST_STRONG_PREP;
	HIP_TRY(c, hipEventCreate(&prep.a));
	HIP_TRY(c, hipEventCreate(&prep.b));
	HIP_TRY(c, hipEventRecord(prep.a, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->planes_snap, c->planes, c->L * 16, hipMemcpyDeviceToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(c->costs_snap, c->costs, c->L * 4, hipMemcpyDeviceToDevice, c->stream));
	ensure_strong_split_buffers(c);   // (before the first launch that takes c->d)
	hipLaunchKernelGGL(dvp_strong_search, dim3(g.grid()), dim3(256), 0, c->stream, c->d, a);
	if (strong_form(c->sw, c->NI - 1, c->split_fits, c->d.reuse_hdr != nullptr, 0).plan) hipLaunchKernelGGL(dvp_strong_plan, dim3(g.grid()), dim3(256), 0, c->stream, c->d, a);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(prep.b, c->stream));
	c->events.push_back(prep);
	return 0;
}

static int launch_strong_update(dvp_ctx* c, const LaunchGeom& g, const LaunchArgs& a) {
	const dim3 grid(g.grid()), block(256);
	const dim3 wave_grid((unsigned)((g.grid() + 7) / 8 * 32)), wave_block(64);   // DVP_KERNEL64 launch sites: four one-wave workgroups per tile
	ensure_strong_split_buffers(c);
	const StrongForm f = strong_form(c->sw, c->NI - 1, c->split_fits, c->d.reuse_hdr != nullptr, (unsigned long long)c->pitch * (c->H + 2 * kImgPad) * 8 * c->NI);
	switch (f.kernel) {
	case STRONG_SPLIT:
		if (f.eval_items) hipLaunchKernelGGL(DVP_PICK(dvp_strong_eval_items, ), wave_grid, wave_block, 0, c->stream, c->d, a);
		else hipLaunchKernelGGL(DVP_PICK(dvp_strong_eval, ), wave_grid, wave_block, 0, c->stream, c->d, a);
		hipLaunchKernelGGL(f.decide == 4 ? dvp_strong_decide_v4 : f.decide == 6 ? dvp_strong_decide_v6 : f.decide == 8 ? dvp_strong_decide_v8 : f.decide == 10 ? dvp_strong_decide_v10 :
		                   f.decide == 12 ? dvp_strong_decide_v12 : f.decide == 16 ? dvp_strong_decide_v16 : dvp_strong_decide_wide, grid, block, 0, c->stream, c->d, a);
		// lanes: every lane on its own (hypothesis, view) sequence; the lanes' image planes are 32-bit byte offsets from the set's base
		if (f.refine_lanes) hipLaunchKernelGGL(DVP_PICK(dvp_strong_refine_lanes, ), wave_grid, wave_block, 0, c->stream, c->d, a);
		else hipLaunchKernelGGL(DVP_PICK(dvp_strong_refine, ), wave_grid, wave_block, 0, c->stream, c->d, a);
		break;
	case STRONG_MONO_V8: hipLaunchKernelGGL(DVP_PICK(dvp_strong_update_v8, ), grid, block, 0, c->stream, c->d, a); break;
	case STRONG_MONO_V16: hipLaunchKernelGGL(DVP_PICK(dvp_strong_update_v16, ), grid, block, 0, c->stream, c->d, a); break;
	case STRONG_MONO: hipLaunchKernelGGL(DVP_PICK(dvp_strong_update, ), grid, block, 0, c->stream, c->d, a); break;
	}
	HIP_TRY(c, hipGetLastError());
	return 0;
}

static int launch_weak_update(dvp_ctx* c, ListArgs la) {
	if (ensure_anchor_table(c, la.covered_rows)) return 1;
	if (c->d.anchor_tab && grow_weak_phase_buffers(c, (size_t)(c->d.weak_black + c->d.weak_red))) return 1;
	const WeakForm f = weak_form(c->sw, c->d.anchor_tab != nullptr, c->weak_phase_fits, la.count);
	const int fmt = dvp_image_format(c);
	const dim3 lg((la.count + 255) / 256), block(256), w64(64), lg64((la.count + 63) / 64);
	switch (f.kernel) {
	case WEAK_PHASED:
#define DVP_GROUP_LAUNCH(NAME, PHASE) { la.group = f.group[PHASE]; la.run = f.run[PHASE]; hipLaunchKernelGGL(DVP_PICK_FMT(NAME, ), dim3((la.count + la.group - 1) / la.group), w64, 0, c->stream, c->d, la); }
		DVP_GROUP_LAUNCH(dvp_weak_eval_candidates, 0)
		hipLaunchKernelGGL(dvp_weak_select_views, lg, block, 0, c->stream, c->d, la);
		DVP_GROUP_LAUNCH(dvp_weak_eval_planes, 1)
		hipLaunchKernelGGL(dvp_weak_make_hypotheses, lg, block, 0, c->stream, c->d, la);
		DVP_GROUP_LAUNCH(dvp_weak_eval_first_view, 2)
		DVP_GROUP_LAUNCH(dvp_weak_eval_survivors, 3)
#undef DVP_GROUP_LAUNCH
		hipLaunchKernelGGL(dvp_weak_adopt, lg, block, 0, c->stream, c->d, la);
		hipLaunchKernelGGL(DVP_PICK(dvp_weak_final_cost, ), lg64, w64, 0, c->stream, c->d, la);
		break;
	case WEAK_WAVE: hipLaunchKernelGGL(DVP_PICK_FMT(dvp_weak_update_wave, ), dim3(la.count), w64, 0, c->stream, c->d, la); break;
	case WEAK_WAVE_NOTAB: hipLaunchKernelGGL(DVP_PICK_FMT(dvp_weak_update_wave, _notab), dim3(la.count), w64, 0, c->stream, c->d, la); break;
	}
	return 0;
}

// weak-path launch sites: lane-per-WEAK-pixel.  Non-WEAK pixels' outputs of these kernels are
// constants / copies and are produced by plain fills: weak_nearest_strong = (-1,-1)
// (APD.cu:4169-4173), fit plane = plane (APD.cu:4208-4211).
static int launch_list_site(dvp_ctx* c, int stage, int iter, int colour) {
	const dim3 block(256);
	const size_t words = edge_bits_words(c->W, c->H);
	const dim3 wgrid((unsigned)((words + 255) / 256));
	if (stage == DVP_ST_FIND_NEAREST_STRONG && c->d.weak_black + c->d.weak_red > 0) {   // its ring search reads row and column segments of the STRONG map
		hipLaunchKernelGGL(dvp_pack_edge_bits, wgrid, block, 0, c->stream, c->weak_info, c->strong_bits, c->W, c->H, edge_tiles_x(c->W), words, (int)DVP_STRONG);
		hipLaunchKernelGGL(dvp_pack_bits_transposed, wgrid, block, 0, c->stream, c->weak_info, c->strong_bits_t, c->W, c->H, edge_tiles_x(c->W), words, (int)DVP_STRONG);
		HIP_TRY(c, hipGetLastError());
	}
	if (stage == DVP_ST_GEN_NEIGHBOURS || stage == DVP_ST_RANSAC_FIT) {   // the launch sites that walk lines over the edge map
		hipLaunchKernelGGL(dvp_pack_edge_bits, wgrid, block, 0, c->stream, c->edge, c->edge_bits, c->W, c->H, edge_tiles_x(c->W), words, -1);
		HIP_TRY(c, hipGetLastError());
		const int cells = c->d.sat_cells_x * c->d.sat_cells_y;
		hipLaunchKernelGGL(dvp_edge_cell_counts, dim3((cells + 255) / 256), dim3(256), 0, c->stream, c->d);
		hipLaunchKernelGGL(dvp_edge_sat_rows, dim3((c->d.sat_cells_y + 1 + 63) / 64), dim3(64), 0, c->stream, c->d);
		hipLaunchKernelGGL(dvp_edge_sat_cols, dim3((c->d.sat_cells_x + 1 + 63) / 64), dim3(64), 0, c->stream, c->d);
		HIP_TRY(c, hipGetLastError());
		if (stage == DVP_ST_GEN_NEIGHBOURS) {   // its anchor search probes "is this pixel STRONG" all over the image
			hipLaunchKernelGGL(dvp_pack_edge_bits, wgrid, block, 0, c->stream, c->weak_info, c->strong_bits, c->W, c->H, edge_tiles_x(c->W), words, (int)DVP_STRONG);
			HIP_TRY(c, hipGetLastError());
		}
	}
	if (stage == DVP_ST_FIND_NEAREST_STRONG) HIP_TRY(c, hipMemsetAsync(c->weak_nearest_strong, 0xFF, c->L * sizeof(s2), c->stream));
	if (stage == DVP_ST_RANSAC_FIT) HIP_TRY(c, hipMemcpyAsync(c->fit_planes, c->planes, c->L * 16, hipMemcpyDeviceToDevice, c->stream));
	ListArgs la;
	la.iter = iter;
	la.covered_rows = 2 * make_geom(c->W, c->H, true).rows;
	la.base = (stage == DVP_ST_WEAK_UPDATE && colour == 1) ? c->d.weak_black : 0;
	la.count = (stage == DVP_ST_WEAK_UPDATE) ? (colour == 0 ? c->d.weak_black : (colour == 1 ? c->d.weak_red : c->d.weak_black + c->d.weak_red)) : c->d.weak_black + c->d.weak_red;   // colour 2 (dvp_run_patchmatch): both colours of the weak update in one launch site
	if (la.count <= 0) return 0;
	const dim3 lg((la.count + 255) / 256);
	switch (stage) {
	case DVP_ST_FIND_NEAREST_STRONG: hipLaunchKernelGGL(DVP_PICK(dvp_find_nearest_strong_list, ), lg, block, 0, c->stream, c->d, la); break;
	case DVP_ST_GEN_NEIGHBOURS:
		if (c->sw.gn_wave) hipLaunchKernelGGL(dvp_gen_neighbours_search, dim3((la.count + 3) / 4), block, 0, c->stream, c->d, la);
		else hipLaunchKernelGGL(dvp_gen_neighbours_list, lg, block, 0, c->stream, c->d, la);
		hipLaunchKernelGGL(dvp_gen_neighbours_fit, dim3(la.count), dim3(64), 0, c->stream, c->d, la);
		break;
	case DVP_ST_NEIGHBOUR_UPDATE: hipLaunchKernelGGL(DVP_PICK(dvp_neighbour_update_list, ), lg, block, 0, c->stream, c->d, la); break;
	case DVP_ST_RANSAC_FIT:
		if (c->sw.ransac_wave) hipLaunchKernelGGL(dvp_ransac_fit_plane_wave, dim3(la.count), dim3(64), 0, c->stream, c->d, la);
		else hipLaunchKernelGGL(DVP_PICK(dvp_ransac_fit_plane_list, ), lg, block, 0, c->stream, c->d, la);
		break;
	case DVP_ST_WEAK_UPDATE:
		if (launch_weak_update(c, la)) return 1;
		break;
	}
	HIP_TRY(c, hipGetLastError());
	return 0;
}

// DepthToWeak, with LocalRefine when `fused`: the two separate kernels, the fused one, or the view-compacted passes
static int launch_sweeps(dvp_ctx* c, const LaunchGeom& g, const LaunchArgs& a, bool fused) {
	const dim3 grid(g.grid()), block(256);
	if (sweep_form(c->sw, fused, c->d.params, c->sweep_fits, c->W, c->H).kernel == SWEEP_PASSES) ensure_sweep_buffers(c);
	const SweepForm f = sweep_form(c->sw, fused, c->d.params, c->sweep_fits, c->W, c->H);
	if (sweep_eval_form(c->sw, f, c->sweep_list_fits) == SWEEP_EVAL_LISTS) ensure_sweep_list_buffers(c);
	if (f.kernel == SWEEP_PASSES) {
		const bool lists = sweep_eval_form(c->sw, f, c->sweep_list_fits) == SWEEP_EVAL_LISTS;
		const auto list_eval = c->sw.sweep_all_slots ? DVP_PICK(dvp_sweep_eval_list, _all) : DVP_PICK(dvp_sweep_eval_list, );
		LaunchArgs s0 = a, s1 = a, sb = a;
		s0.iter = 0; s1.iter = 1; sb.iter = kSweepBorderOnly;
		const int etx = (c->W + 63) / 64, ety = (c->H + kSweepRows - 1) / kSweepRows;
		s0.tiles_x = s1.tiles_x = etx; s0.tiles = s1.tiles = etx * ety;
		const dim3 egrid((unsigned)(etx * ety), (unsigned)(c->NI - 1));
		hipLaunchKernelGGL(dvp_sweep_prepare, grid, block, 0, c->stream, c->d, a);
		// evaluate / decide / evaluate / decide over the whole image, or band of rows after band of rows through the one band-sized
		// cost buffer (every pass is per pixel: same bits)
		const int band_rows = c->sweep_band_rows > 0 ? c->sweep_band_rows : c->H;
		for (int row0 = 0; row0 < c->H; row0 += band_rows) {
			Dev db = c->d;
			LaunchArgs b0 = s0, b1 = s1;
			dim3 bgrid = egrid;
			b0.rows = b1.rows = 0;
			if (c->sweep_band_rows > 0) {
				const int row1 = std::min(c->H, row0 + band_rows);
				db.sweep_px0 = row0 * c->W; db.sweep_row0 = row0; db.sweep_row1 = row1;
				const int bty = (row1 - row0 + kSweepRows - 1) / kSweepRows;
				b0.rows = b1.rows = row0 / kSweepRows;
				b0.tiles = b1.tiles = etx * bty;
				bgrid = dim3((unsigned)(etx * bty), (unsigned)(c->NI - 1));
			}
			if (lists) {
				// per stage: the band's lists (counts per (view, tile), a scan per view — dvp_scan3 takes three — and the scatter), then
				// the evaluation over the upper bound of the lists' lengths, which stay on the device
				const int S = c->NI - 1, T = b0.tiles;
				const dim3 tgrid((unsigned)((T + 3) / 4)), lgrid((unsigned)sweep_list_grid(c->sweep_list_cap, kSweepListRounds), (unsigned)S);
				for (int stage = 0; stage < (f.second_eval ? 2 : 1); ++stage) {
					const LaunchArgs& bs = stage ? b1 : b0;
					hipLaunchKernelGGL(dvp_sweep_list_counts, tgrid, block, 0, c->stream, db, bs);
					for (int v0 = 0; v0 < S; v0 += 3)
						hipLaunchKernelGGL(dvp_scan3, dim3(3), dim3(1024), 0, c->stream, db.sweep_list_counts, v0 * T, std::min(v0 + 1, S) * T, std::min(v0 + 2, S) * T, std::min(v0 + 3, S) * T, db.sweep_list_n + v0);
					hipLaunchKernelGGL(dvp_sweep_list_fill, tgrid, block, 0, c->stream, db, bs);
					hipLaunchKernelGGL(list_eval, lgrid, dim3(64), 0, c->stream, db, bs);
					if (stage == 0) hipLaunchKernelGGL(dvp_sweep_decide1, grid, block, 0, c->stream, db, a);
				}
				hipLaunchKernelGGL(dvp_sweep_decide2, grid, block, 0, c->stream, db, a);
				continue;
			}
			const auto eval = c->sw.sweep_all_slots ? DVP_PICK(dvp_sweep_eval, _all) : DVP_PICK(dvp_sweep_eval, );
			hipLaunchKernelGGL(eval, bgrid, dim3(64), 0, c->stream, db, b0);
			hipLaunchKernelGGL(dvp_sweep_decide1, grid, block, 0, c->stream, db, a);
			if (f.second_eval) hipLaunchKernelGGL(eval, bgrid, dim3(64), 0, c->stream, db, b1);
			hipLaunchKernelGGL(dvp_sweep_decide2, grid, block, 0, c->stream, db, a);
		}
		if (f.border_kernel) {
			const long long frame = 12ll * c->W + 12ll * (c->H - 12);
			hipLaunchKernelGGL(DVP_PICK(dvp_sweep_border, ), dim3((unsigned)((frame + 63) / 64)), dim3(64), 0, c->stream, c->d, sb);
		}
		else hipLaunchKernelGGL(DVP_PICK(dvp_depth_to_weak_refine, ), grid, block, 0, c->stream, c->d, sb);
	}
	else if (f.kernel == SWEEP_FUSED) hipLaunchKernelGGL(DVP_PICK(dvp_depth_to_weak_refine, ), grid, block, 0, c->stream, c->d, a);
	else hipLaunchKernelGGL(DVP_PICK(dvp_depth_to_weak, ), grid, block, 0, c->stream, c->d, a);
	HIP_TRY(c, hipGetLastError());
	return 0;
}

// the launch sites of one kernel over the image's pixels
static int launch_pixel_site(dvp_ctx* c, int stage, const LaunchGeom& g, const LaunchArgs& a, bool fused) {
	const dim3 grid(g.grid()), block(256);
	if (stage == DVP_ST_GEN_EDGE_INFORM && c->d.params.use_edge) {
		hipLaunchKernelGGL(dvp_edge_rays, dim3((c->W + c->H + 255) / 256, 8), dim3(256), 0, c->stream, c->d, 0);
		HIP_TRY(c, hipGetLastError());
	}
	if (stage == DVP_ST_GEN_EDGE_INFORM && c->d.params.use_label && c->d.weak_count > 0) {   // label boundaries are searched for WEAK pixels only
		if (!c->label_stop) {
			if (dalloc(c, &c->label_stop, c->L * 8, false)) return 1;
			sync_dev_struct(c);
		}
		hipLaunchKernelGGL(dvp_edge_rays, dim3((c->W + c->H + 255) / 256, 8), dim3(256), 0, c->stream, c->d, 1);
		HIP_TRY(c, hipGetLastError());
	}
	switch (stage) {
	case DVP_ST_GEN_EDGE_INFORM:
		if (!fused) launch_gen_candidates(c, c->stream, c->d, g.grid(), a);   // fused: dvp_run_patchmatch issued them on the side stream
		hipLaunchKernelGGL(DVP_PICK(dvp_gen_edge_inform, ), grid, block, 0, c->stream, c->d, a);
		break;
	case DVP_ST_RANDOM_INIT: hipLaunchKernelGGL(DVP_PICK(dvp_random_init, ), grid, block, 0, c->stream, c->d, a); break;
	case DVP_ST_GET_DEPTH_NORMAL: hipLaunchKernelGGL(DVP_PICK(dvp_get_depth_normal, ), grid, block, 0, c->stream, c->d, a); break;
	case DVP_ST_FILTER_STRONG: hipLaunchKernelGGL(DVP_PICK(dvp_filter_strong, ), grid, block, 0, c->stream, c->d, a); break;
	case DVP_ST_LOCAL_REFINE: hipLaunchKernelGGL(DVP_PICK(dvp_local_refine, ), grid, block, 0, c->stream, c->d, a); break;
	}
	HIP_TRY(c, hipGetLastError());
	return 0;
}

static int launch_stage(dvp_ctx* c, int stage, int iter, int colour, bool fused = false) {
	if (stage < 0 || stage >= DVP_ST_LAUNCHABLE) { c->error = "bad stage id"; return 1; }
	if (!c->sector_taps) { c->error = "dvp_set_params must be called before running kernels"; return 1; }
	if (c->d.params.geom_consistency && !c->have_depths) { c->error = "geom_consistency is on but no depth maps were uploaded"; return 1; }
	const LaunchGeom g = make_geom(c->W, c->H, stage_is_half(stage));
	const LaunchArgs a = make_args(g, colour, iter);
	if (c->events.size() >= 2048 && dvp_get_timings(c, nullptr)) return 1;   // fold pending timings: bounds the event pool
	if (stage != DVP_ST_STRONG_UPDATE && stage != DVP_ST_RANSAC_FIT && stage != DVP_ST_WEAK_UPDATE) c->anchor_tab_valid = false;   // anchors / offsets / WEAK states may change: the next weak update rebuilds its table
	if (stage == DVP_ST_STRONG_UPDATE && launch_strong_prep(c, g, a)) return 1;
	EventPair ep;
	ep.stage = stage;
	HIP_TRY(c, hipEventCreate(&ep.a));
	HIP_TRY(c, hipEventCreate(&ep.b));
	if (c->profiling) HIP_TRY(c, hipMemsetAsync(c->eval_counter, 0, 8, c->stream));
	HIP_TRY(c, hipEventRecord(ep.a, c->stream));
	int r;
	switch (stage) {
	case DVP_ST_FIND_NEAREST_STRONG: case DVP_ST_GEN_NEIGHBOURS: case DVP_ST_NEIGHBOUR_UPDATE: case DVP_ST_RANSAC_FIT: case DVP_ST_WEAK_UPDATE:
		r = launch_list_site(c, stage, iter, colour); break;
	case DVP_ST_STRONG_UPDATE: r = launch_strong_update(c, g, a); break;
	case DVP_ST_DEPTH_TO_WEAK: r = launch_sweeps(c, g, a, fused); break;
	default: r = launch_pixel_site(c, stage, g, a, fused); break;
	}
	if (r) return 1;
	HIP_TRY(c, hipEventRecord(ep.b, c->stream));
	c->events.push_back(ep);
	if (c->profiling) {
		unsigned long long n = 0;
		HIP_TRY(c, hipMemcpyAsync(&n, c->eval_counter, 8, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		c->timings.ncc_evals[stage] += n;
	}
	return 0;
}

int dvp_run_stage(dvp_ctx* c, int stage, int iter, int colour) {
	if (set_device(c)) return 1;
	return launch_stage(c, stage, iter, colour);
}

// scratch + the first `slots` output maps of dvp_edge_map_begin
static int ensure_edge_buffers(dvp_ctx* c, int slots) {
	if (dvpedge::scratch_reserve(c->eg, c->L)) { c->error = "dvp_edge_map: out of device memory"; return 1; }
	for (int k = 0; k < slots; ++k) {
		dvp_ctx::EdgeSlot& sl = c->eg_slot[k];
		if (sl.map.reserve(c->L)) { c->error = "dvp_edge_map: out of device memory"; return 1; }
		if (!sl.done && hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); sl.done = nullptr; c->error = "dvp_edge_map: hipEventCreate failed"; return 1; }
	}
	return 0;
}

// Optional buffers ahead of their first use (a helper thread of the driver calls this on the context it prepares for the next
// pyramid level): flags bit 0 = the split strong update's cost block, bit 1 = the view-compacted sweep passes' buffers;
// weak_pixels > 0: anchor table and hand-over buffers of the weak update for that many WEAK pixels.  Nothing here is required —
// every launch site allocates what it lacks — and a buffer that does not fit selects the fall-back form exactly as there.
int dvp_ctx_reserve(dvp_ctx* c, int weak_pixels, int flags) {
	if (set_device(c)) return 1;
	if (flags & 1) ensure_strong_split_buffers(c);
	if (flags & 2) { ensure_sweep_buffers(c); ensure_sweep_list_buffers(c); }
	if ((flags & 4) && !c->sw.no_images8 && !c->sw.no_images16 && ensure_images16(c)) return 1;
	if ((flags & 8) && ensure_edge_buffers(c, 2)) return 1;
	if ((flags & 16) && dvpvc::scratch_reserve(c->vc, c->L, c->NI - 1)) { c->error = "dvp_ctx_reserve: out of device memory (view clean-up)"; return 1; }
	if (weak_pixels > 0) {
		const size_t wc = std::min<size_t>((size_t)weak_pixels, c->L);
		if (grow_anchor_table(c, wc)) return 1;
		if (c->anchor_tab && grow_weak_phase_buffers(c, wc)) return 1;
		c->anchor_tab_valid = false;
	}
	return 0;
}

int dvp_synchronize(dvp_ctx* c) {
	if (set_device(c)) return 1;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return 0;
}

// APD::RunPatchMatch (APD.cu:4406-4532): same launch order; no host sync between launches.
int dvp_run_patchmatch(dvp_ctx* c) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	EventPair tot, itl;
	tot.stage = EV_TOTAL; itl.stage = EV_ITER_LOOP;
	HIP_TRY(c, hipEventCreate(&tot.a)); HIP_TRY(c, hipEventCreate(&tot.b));
	HIP_TRY(c, hipEventCreate(&itl.a)); HIP_TRY(c, hipEventCreate(&itl.b));
	HIP_TRY(c, hipEventRecord(tot.a, c->stream));
	// The candidates read the images, the sector tables and selected_views (which RandomInitialization is the first
	// to write) and are read by the weak updates: they run on the side stream from here to just before RandomInit.
	const bool side_work = c->d.weak_count > 0;
	if (candidates_masked(c->sw, c->d.weak_count, c->L, c->cand_mask_fits) && !c->cand_mask)   // mark bytes, anchor list, snapshot of the selected-view map: 9 bytes per pixel
		alloc_group_or_fall_back(c, { areq(&c->cand_mask, c->L), areq(&c->cand_list, c->L * 4), areq(&c->cand_n, 4), areq(&c->sel_snap, (c->L + c->W) * 4) },
			nullptr, &c->cand_mask_fits, nullptr, 0.0);   // no room: every pixel, as before
	const bool masked = candidates_masked(c->sw, c->d.weak_count, c->L, c->cand_mask_fits);
	if (side_work && !masked) {
		if (!c->sector_taps) { c->error = "dvp_set_params must be called before running kernels"; return 1; }
		HIP_TRY(c, hipEventRecord(c->side_fork, c->stream));
		HIP_TRY(c, hipStreamWaitEvent(c->side, c->side_fork, 0));
		const LaunchGeom g = make_geom(c->W, c->H, false);
		launch_gen_candidates(c, c->side, c->d, g.grid(), make_args(g, 0, 0));
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipEventRecord(c->side_join, c->side));
	}
	if (launch_stage(c, DVP_ST_GEN_EDGE_INFORM, 0, 0, true)) return 1;
	if (launch_stage(c, DVP_ST_FIND_NEAREST_STRONG, 0, 0)) return 1;
	if (launch_stage(c, DVP_ST_GEN_NEIGHBOURS, 0, 0)) return 1;
	if (launch_stage(c, DVP_ST_NEIGHBOUR_UPDATE, 0, 0)) return 1;
	if (side_work && !masked) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->side_join, 0));
	if (masked) {
		// the anchors are known now; RandomInitialization is the first to rewrite the selected views the candidates read: they
		// get a snapshot and run beside RandomInit and the first strong updates, joined in front of the first weak update
		if (!c->sector_taps) { c->error = "dvp_set_params must be called before running kernels"; return 1; }
		HIP_TRY(c, hipMemcpyAsync(c->sel_snap, c->selected_views, (c->L + c->W) * 4, hipMemcpyDeviceToDevice, c->stream));
		HIP_TRY(c, hipEventRecord(c->side_fork, c->stream));
		HIP_TRY(c, hipStreamWaitEvent(c->side, c->side_fork, 0));
		HIP_TRY(c, hipMemsetAsync(c->cand_mask, 0, c->L, c->side));
		HIP_TRY(c, hipMemsetAsync(c->cand_n, 0, 4, c->side));
		ListArgs la;
		la.base = 0; la.count = c->d.weak_black + c->d.weak_red; la.iter = 0; la.covered_rows = 0; la.group = 1; la.run = 1;
		if (la.count > 0) hipLaunchKernelGGL(dvp_anchor_mask, dim3((la.count + 255) / 256), dim3(256), 0, c->side, c->d, la, c->cand_mask);
		hipLaunchKernelGGL(dvp_mask_compact, dim3((unsigned)((c->L + 255) / 256)), dim3(256), 0, c->side, c->cand_mask, c->L, c->cand_list, c->cand_n);
		// (the list's length stays on the device: the grid covers the at most 11 anchors per WEAK pixel, blocks past the end leave)
		const size_t most = std::min(c->L, (size_t)la.count * (DVP_NEIGHBOUR_NUM - 1));
		Dev dsnap = c->d;
		dsnap.selected_views = c->sel_snap;
		if (most > 0) launch_gen_candidates(c, c->side, dsnap, (unsigned)((most + 255) / 256), LaunchArgs{}, c->cand_list, c->cand_n);
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipEventRecord(c->side_join, c->side));
	}
	if (launch_stage(c, DVP_ST_RANDOM_INIT, 0, 0)) return 1;
	HIP_TRY(c, hipEventRecord(itl.a, c->stream));
	for (int i = 0; i < c->d.params.max_iterations; ++i) {
		if (launch_stage(c, DVP_ST_STRONG_UPDATE, i, 0)) return 1;
		if (launch_stage(c, DVP_ST_STRONG_UPDATE, i, 1)) return 1;
		// without WEAK pixels the three weak-path launches of an iteration do nothing but RANSACToGetFitPlane's copy
		// fit plane = plane (APD.cu:4208-4211), which only the last iteration's launch leaves behind
		if (c->d.weak_count == 0 && i == c->d.params.max_iterations - 1)
			HIP_TRY(c, hipMemcpyAsync(c->fit_planes, c->planes, c->L * 16, hipMemcpyDeviceToDevice, c->stream));
		if (c->d.weak_count > 0) {   // these three only touch WEAK pixels
			if (masked && i == 0) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->side_join, 0));   // the anchors' candidate records
			if (launch_stage(c, DVP_ST_RANSAC_FIT, i, 0)) return 1;
			// Black then red (APD.cu:4487-4489).  A WEAK pixel's update reads other pixels' state only at its anchors, which are STRONG
			// (GenNeighbours) and which no weak update writes: the two launches commute, and as the eight launches of the phased form
			// they are issued once over the whole WEAK list (half the launches and their tails).  dvp_run_stage keeps the colours apart.
			if (weak_joins_colours(c->sw, c->anchor_tab_fits, c->weak_phase_fits)) {
				if (launch_stage(c, DVP_ST_WEAK_UPDATE, i, 2)) return 1;
			} else {
				if (launch_stage(c, DVP_ST_WEAK_UPDATE, i, 0)) return 1;
				if (launch_stage(c, DVP_ST_WEAK_UPDATE, i, 1)) return 1;
			}
		}
	}
	if (masked && c->d.params.max_iterations <= 0) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->side_join, 0));
	HIP_TRY(c, hipEventRecord(itl.b, c->stream));
	if (launch_stage(c, DVP_ST_GET_DEPTH_NORMAL, 0, 0)) return 1;
	if (launch_stage(c, DVP_ST_FILTER_STRONG, 0, 0)) return 1;
	if (launch_stage(c, DVP_ST_FILTER_STRONG, 0, 1)) return 1;
	// DepthToWeak and LocalRefine (APD.cu:4502-4505) in ONE launch: LocalRefine's sweep repeats eleven planes of
	// DepthToWeak's (dvp_sweep.hpp, depth_to_weak_px).  Timed in the DVP_ST_DEPTH_TO_WEAK bucket.
	if (launch_stage(c, DVP_ST_DEPTH_TO_WEAK, 0, 0, true)) return 1;
	HIP_TRY(c, hipEventRecord(tot.b, c->stream));
	c->events.push_back(tot);
	c->events.push_back(itl);
	return 0;
}

// ---- results ----------------------------------------------------------------------------------
int dvp_download_state(dvp_ctx* c, float* planes, uint32_t* views, uint8_t* weak, int32_t* radius) {
	if (set_device(c)) return 1;
	const size_t L = c->L;
	if (planes) HIP_TRY(c, hipMemcpyAsync(planes, c->planes, L * 16, hipMemcpyDeviceToHost, c->stream));
	if (views) HIP_TRY(c, hipMemcpyAsync(views, c->selected_views, L * 4, hipMemcpyDeviceToHost, c->stream));
	if (weak) HIP_TRY(c, hipMemcpyAsync(weak, c->weak_info, L, hipMemcpyDeviceToHost, c->stream));
	if (radius) HIP_TRY(c, hipMemcpyAsync(radius, c->radius, L * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return 0;
}

static void download_done(dvp_ctx* c) {
	{ std::lock_guard<std::mutex> lk(c->dl_m); c->dl_busy = false; c->dl_fetching = false; }
	c->dl_cv.notify_all();
}
int dvp_download_maps_begin(dvp_ctx* c, float* depth_device_copy) {
	if (set_device(c)) return 1;
	{   // the previous view's maps must have been fetched: its background job may not even have started yet, so this waits —
		// but not for ever (a second _begin after a _finish that never comes would otherwise hang the driver thread)
		int limit_s = 120;
		if (const char* e = getenv("DVP_DOWNLOAD_WAIT_S")) limit_s = atoi(e);
		std::unique_lock<std::mutex> lk(c->dl_m);
		if (!c->dl_cv.wait_for(lk, std::chrono::seconds(limit_s > 0 ? limit_s : 1), [c] { return !c->dl_busy; })) {
			c->error = "dvp_download_maps_begin: the maps staged by the previous dvp_download_maps_begin were never fetched (dvp_download_maps_finish)";
			return 1;
		}
		c->dl_busy = true;
	}
	const size_t L = c->L;
	auto fail = [c]() { download_done(c); return 1; };
	if (!c->maps_out && dalloc(c, &c->maps_out, L * 25, false)) return fail();
	float* d_depth = reinterpret_cast<float*>(c->maps_out);
	float* d_normal = d_depth + L;
	uint8_t* d_state = c->maps_out + L * 24;
	uint32_t* d_views = reinterpret_cast<uint32_t*>(c->maps_out + L * 16);
	hipLaunchKernelGGL(dvp_unpack_maps, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, c->stream, c->planes, c->weak_info, L, c->d.params.depth_min, c->d.params.depth_max,
	                   d_depth, d_normal, d_state);
	if (hipGetLastError() != hipSuccess) { c->error = "dvp_download_maps_begin: launch failed"; return fail(); }
	// the view maps and the radius map are live state: the next view's uploads overwrite them
	if (c->vc_on) {   // dvp_set_view_cleanup: the staged words are the cleaned ones; the device state keeps the raw ones
		if (dvpvc::scratch_reserve(c->vc, L, c->vc_num_src)) { c->error = "dvp_download_maps_begin: out of device memory (view clean-up)"; return fail(); }
		if (dvpvc::launch_clean(c->stream, c->vc, c->selected_views, c->W, c->H, c->vc_num_src, c->vc_min_region, d_views)) { c->error = "dvp_download_maps_begin: launch failed (view clean-up)"; return fail(); }
	}
	if ((!c->vc_on && hipMemcpyAsync(d_views, c->selected_views, L * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) ||
	    hipMemcpyAsync(c->maps_out + L * 20, c->radius, L * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
	    (depth_device_copy && hipMemcpyAsync(depth_device_copy, d_depth, L * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) ||
	    hipStreamSynchronize(c->stream) != hipSuccess) { c->error = "dvp_download_maps_begin: device copies failed"; return fail(); }
	return 0;
}
int dvp_download_maps_finish(dvp_ctx* c, float* depth, float* normal_xyz, uint32_t* views, uint8_t* weak, int32_t* radius) {
	t_finish_error.c = c;
	t_finish_error.msg.clear();
	{
		std::lock_guard<std::mutex> lk(c->dl_m);
		if (!c->dl_busy || c->dl_fetching) { t_finish_error.msg = "dvp_download_maps_finish without dvp_download_maps_begin"; return 1; }
		c->dl_fetching = true;
	}
	auto fail = [c](const char* what) { t_finish_error.msg = what; download_done(c); return 1; };
	if (hipSetDevice(c->device) != hipSuccess) return fail("hipSetDevice failed");
	if (!depth || !normal_xyz || !weak) return fail("dvp_download_maps: depth, normal and weak_info are required");
	if (!c->copy && hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
	const size_t L = c->L;
	// One DMA into pinned memory, then plain copies into the caller's (pageable) maps.  Copies straight into pageable memory go
	// through the runtime's staging path: at 6208x4128 they took 45-50 ms instead of 13 and the driver thread's own uploads for
	// the next view waited behind them (profiles/r05_ab_notes.txt).
	if (!c->maps_host && hipHostMalloc(reinterpret_cast<void**>(&c->maps_host), L * 25, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); c->maps_host = nullptr; }
	if (c->maps_host) {
		if (hipMemcpyAsync(c->maps_host, c->maps_out, L * 25, hipMemcpyDeviceToHost, c->copy) != hipSuccess || hipStreamSynchronize(c->copy) != hipSuccess)
			return fail("dvp_download_maps_finish: copy to the host failed");
		struct Part { void* dst; size_t off, bytes; };
		const Part parts[5] = { { depth, 0, L * 4 }, { normal_xyz, L * 4, L * 12 }, { weak, L * 24, L }, { views, L * 16, L * 4 }, { radius, L * 20, L * 4 } };
		std::vector<std::thread> team;
		const uint8_t* src = c->maps_host;
		for (const Part& pt : parts) {
			if (!pt.dst) continue;
			const size_t chunk = (size_t)32 << 20;
			if (pt.bytes <= chunk) { std::memcpy(pt.dst, src + pt.off, pt.bytes); continue; }
			const int nt = (int)std::min<size_t>(4, (pt.bytes + chunk - 1) / chunk);
			for (int t = 0; t < nt; ++t) {
				const size_t b0 = pt.bytes * t / nt, b1 = pt.bytes * (t + 1) / nt;
				team.emplace_back([=]() { std::memcpy(static_cast<uint8_t*>(pt.dst) + b0, src + pt.off + b0, b1 - b0); });
			}
		}
		for (std::thread& t : team) t.join();
		download_done(c);
		return 0;
	}
	const uint8_t* m = c->maps_out;
	if (hipMemcpyAsync(depth, m, L * 4, hipMemcpyDeviceToHost, c->copy) != hipSuccess ||
	    hipMemcpyAsync(normal_xyz, m + L * 4, L * 12, hipMemcpyDeviceToHost, c->copy) != hipSuccess ||
	    hipMemcpyAsync(weak, m + L * 24, L, hipMemcpyDeviceToHost, c->copy) != hipSuccess ||
	    (views && hipMemcpyAsync(views, m + L * 16, L * 4, hipMemcpyDeviceToHost, c->copy) != hipSuccess) ||
	    (radius && hipMemcpyAsync(radius, m + L * 20, L * 4, hipMemcpyDeviceToHost, c->copy) != hipSuccess) ||
	    hipStreamSynchronize(c->copy) != hipSuccess) return fail("dvp_download_maps_finish: copies to the host failed");
	download_done(c);
	return 0;
}
// ---- the visibility-mask clean-up of the staged words (main.cpp:311-363; dvp_viewclean.hip) ------------------------------------
int dvp_set_view_cleanup(dvp_ctx* c, int enable, int num_src, int min_region) {
	if (enable && (num_src < 0 || num_src > 32)) { c->error = "dvp_set_view_cleanup: num_src must be 0 ... 32 (one bit of a word per source view)"; return 1; }
	c->vc_on = enable != 0;
	c->vc_num_src = enable ? num_src : 0;
	c->vc_min_region = enable ? min_region : 0;
	return 0;
}

// ---- the Canny edge prior from the resident image 0 (EdgeSegment mode 0, APD.cpp:404-466; dvp_edges.hip) ----------------------
int dvp_edge_map_begin(dvp_ctx* c, int install) {
	if (set_device(c)) return 1;
	if (!c->have_images) { c->error = "dvp_edge_map_begin: no images in the context yet (dvp_upload_images)"; return 1; }
	if (c->W < 3 || c->H < 3) { c->error = "dvp_edge_map_begin: width and height must be at least 3"; return 1; }
	int k;
	{   // the slot of this map: a free one, else the older of the two (its map was never fetched)
		std::unique_lock<std::mutex> lk(c->eg_m);
		k = !c->eg_slot[0].pending ? 0 : (!c->eg_slot[1].pending ? 1 : (c->eg_slot[0].seq < c->eg_slot[1].seq ? 0 : 1));
		c->eg_cv.wait(lk, [c, k] { return !c->eg_slot[k].fetching; });   // (a running copy ends in bounded time)
		c->eg_slot[k].pending = false;
	}
	if (ensure_edge_buffers(c, k + 1)) return 1;
	dvp_ctx::EdgeSlot& sl = c->eg_slot[k];
	// image 0 of the row-pair planes: texel (x, y) is the first float of pair (x, y) (dvp_dev.hpp img_texel)
	const float* img0 = c->images + (size_t)c->d.org * 2;
	if (dvpedge::launch_grey_from_float(c->stream, c->eg, img0, (long long)c->pitch, 2, c->W, c->H) || dvpedge::launch_suppress(c->stream, c->eg, c->W, c->H, true) ||
	    dvpedge::launch_hysteresis(c->stream, c->eg, c->W, c->H) || dvpedge::launch_fixups(c->stream, c->eg, c->W, c->H, sl.map.as<uint8_t>(), install ? c->edge : nullptr)) {
		c->error = "dvp_edge_map_begin: launch failed"; return 1;
	}
	HIP_TRY(c, hipEventRecord(sl.done, c->stream));
	std::lock_guard<std::mutex> lk(c->eg_m);
	sl.seq = ++c->eg_seq;
	sl.pending = true;
	return 0;
}

int dvp_edge_map_finish(dvp_ctx* c, uint8_t* edge) {
	t_finish_error.c = c;
	t_finish_error.msg.clear();
	auto fail = [](const char* what) { t_finish_error.msg = what; return 1; };
	if (!edge) return fail("dvp_edge_map_finish: edge is required");
	if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); return fail("dvp_edge_map_finish: hipSetDevice failed"); }
	int k = -1;
	{
		std::lock_guard<std::mutex> lk(c->eg_m);
		for (int i = 0; i < 2; ++i)
			if (c->eg_slot[i].pending && !c->eg_slot[i].fetching && (k < 0 || c->eg_slot[i].seq < c->eg_slot[k].seq)) k = i;
		if (k < 0) return fail("dvp_edge_map_finish: no edge map was begun (dvp_edge_map_begin)");
		c->eg_slot[k].fetching = true;
		if (!c->eg_copy && hipStreamCreateWithFlags(&c->eg_copy, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); c->eg_copy = nullptr; c->eg_slot[k].fetching = false; return fail("dvp_edge_map_finish: hipStreamCreate failed"); }
	}
	dvp_ctx::EdgeSlot& sl = c->eg_slot[k];
	// (two fetches at once share eg_copy: they queue behind each other, each waits for its own copy)
	const bool ok = hipEventSynchronize(sl.done) == hipSuccess && hipMemcpyAsync(edge, sl.map.as<uint8_t>(), c->L, hipMemcpyDeviceToHost, c->eg_copy) == hipSuccess &&
	                hipStreamSynchronize(c->eg_copy) == hipSuccess;
	{
		std::lock_guard<std::mutex> lk(c->eg_m);
		sl.fetching = false;
		sl.pending = false;
	}
	c->eg_cv.notify_all();
	if (!ok) { (void)hipGetLastError(); return fail("dvp_edge_map_finish: copy to the host failed"); }
	return 0;
}

// ---- previews (ShowDepthMap / ShowNormalMap / ShowWeakImage + cv::imwrite, APD.cpp:694-812) ---------------------------------
int dvp_preview_begin(dvp_ctx* c, int kinds, int quality) {
	if (set_device(c)) return 1;
	if (kinds < 1 || kinds > 7) { c->error = "dvp_preview_begin: kinds must be a non-empty set of DVP_PREVIEW_DEPTH | NORMAL | WEAK"; return 1; }
	if (quality < 1 || quality > 100) { c->error = "dvp_preview_begin: quality must be 1..100"; return 1; }
	c->pv_kinds = 0;
	const size_t L = c->L;
	for (int k = 0; k < 3; ++k)
		if ((kinds >> k & 1) && !c->pv_bgr[k] && dalloc(c, &c->pv_bgr[k], L * 3, false)) return 1;
	if (!c->pv_total) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->pv_total), 3 * sizeof(unsigned long long), hipHostMallocDefault));
	if (!c->pv_done) HIP_TRY(c, hipEventCreateWithFlags(&c->pv_done, hipEventDisableTiming));
	if (!c->pv_copy) HIP_TRY(c, hipStreamCreateWithFlags(&c->pv_copy, hipStreamNonBlocking));
	auto bgr = [&](int k) { return (kinds >> k & 1) ? c->pv_bgr[k] : nullptr; };
	if (dvpjpeg::launch_render(c->stream, reinterpret_cast<const float*>(c->planes), c->weak_info, L, c->d.params.depth_min, c->d.params.depth_max,
	                           bgr(0), bgr(1), bgr(2))) { c->error = "dvp_preview_begin: render launch failed"; return 1; }
	for (int k = 0; k < 3; ++k)
		if ((kinds >> k & 1) && dvpjpeg::encode_begin(c->pv_enc[k], c->stream, c->pv_bgr[k], (long long)c->W * 3, c->W, c->H, 3, quality, 0, &c->pv_total[k])) {
			c->error = std::string("dvp_preview_begin: ") + c->pv_enc[k].error; return 1;
		}
	HIP_TRY(c, hipStreamSynchronize(c->stream));   // the one wait: the encodes' sizes
	for (int k = 0; k < 3; ++k)
		if ((kinds >> k & 1) && dvpjpeg::encode_write(c->pv_enc[k], c->stream, c->pv_total[k])) {
			c->error = std::string("dvp_preview_begin: ") + c->pv_enc[k].error; return 1;
		}
	HIP_TRY(c, hipEventRecord(c->pv_done, c->stream));
	c->pv_kinds = kinds;
	return 0;
}
static int preview_slot(dvp_ctx* c, int kind, const char* who) {
	t_finish_error.c = c;
	t_finish_error.msg.clear();
	const int k = kind == DVP_PREVIEW_DEPTH ? 0 : kind == DVP_PREVIEW_NORMAL ? 1 : kind == DVP_PREVIEW_WEAK ? 2 : -1;
	if (k < 0 || !(c->pv_kinds >> k & 1)) { t_finish_error.msg = std::string(who) + ": that preview was not begun (dvp_preview_begin)"; return -1; }
	if (hipSetDevice(c->device) != hipSuccess || hipEventSynchronize(c->pv_done) != hipSuccess) { t_finish_error.msg = std::string(who) + ": device error"; return -1; }
	return k;
}
int dvp_preview_finish(dvp_ctx* c, int kind, uint8_t* dst, long long capacity, long long* bytes) {
	const int k = preview_slot(c, kind, "dvp_preview_finish");
	if (k < 0) return 1;
	const dvpjpeg::Encoder& e = c->pv_enc[k];
	const long long n = (long long)dvpjpeg::file_bytes(e);
	if (bytes) *bytes = n;
	if (!dst || capacity < n) { t_finish_error.msg = "dvp_preview_finish: capacity below the encoded size (*bytes)"; return 1; }
	memcpy(dst, e.header, e.header_len);
	if (hipMemcpyAsync(dst + e.header_len, e.out.as<uint8_t>(), e.data_bytes, hipMemcpyDeviceToHost, c->pv_copy) != hipSuccess || hipStreamSynchronize(c->pv_copy) != hipSuccess) {
		t_finish_error.msg = "dvp_preview_finish: copy to the host failed"; return 1;
	}
	dst[n - 2] = 0xFF;
	dst[n - 1] = 0xD9;
	return 0;
}
int dvp_preview_pixels(dvp_ctx* c, int kind, uint8_t* bgr) {
	const int k = preview_slot(c, kind, "dvp_preview_pixels");
	if (k < 0) return 1;
	if (!bgr || hipMemcpyAsync(bgr, c->pv_bgr[k], c->L * 3, hipMemcpyDeviceToHost, c->pv_copy) != hipSuccess || hipStreamSynchronize(c->pv_copy) != hipSuccess) {
		t_finish_error.msg = "dvp_preview_pixels: copy to the host failed"; return 1;
	}
	return 0;
}

int dvp_download_maps(dvp_ctx* c, float* depth, float* normal_xyz, uint32_t* views, uint8_t* weak, int32_t* radius) {
	if (!depth || !normal_xyz || !weak) { c->error = "dvp_download_maps: depth, normal and weak_info are required"; return 1; }
	if (dvp_download_maps_begin(c, nullptr)) return 1;
	return dvp_download_maps_finish(c, depth, normal_xyz, views, weak, radius);
}

static void* buffer_ptr(dvp_ctx* c, int id, size_t* bytes) {
	const size_t L = c->L, S = (size_t)c->NI - 1;
	const size_t wc = c->d.weak_count > 0 ? (size_t)c->d.weak_count : 1;
	switch (id) {
	case DVP_BUF_PLANES: *bytes = L * 16; return c->planes;
	case DVP_BUF_COSTS: *bytes = L * 4; return c->costs;
	case DVP_BUF_SELECTED_VIEWS: *bytes = L * 4; return c->selected_views;
	case DVP_BUF_VIEW_WEIGHT: *bytes = L * 32; return c->view_weight;
	case DVP_BUF_WEAK_INFO: *bytes = L; return c->weak_info;
	case DVP_BUF_WEAK_RELIABLE: *bytes = L; return c->weak_reliable;
	case DVP_BUF_WEAK_NEAREST_STRONG: *bytes = L * 4; return c->weak_nearest_strong;
	case DVP_BUF_NEIGHBOURS_MAP: *bytes = L * 4; return c->neighbours_map;
	case DVP_BUF_NEIGHBOURS: *bytes = wc * DVP_NEIGHBOUR_NUM * 4; return c->neighbours;
	case DVP_BUF_FIT_PLANES: *bytes = L * 16; return c->fit_planes;
	case DVP_BUF_CANDIDATE: *bytes = L * S * 8 * 4; return c->candidate;
	case DVP_BUF_EDGE: *bytes = L; return c->edge;
	case DVP_BUF_EDGE_NEIGH: *bytes = L * 8 * 4; return c->edge_neigh;
	case DVP_BUF_LABEL: *bytes = L * 4; return c->label;
	case DVP_BUF_LABEL_BOUNDARY: *bytes = wc * 8 * 4; return c->label_boundary;
	case DVP_BUF_COMPLEX: *bytes = wc * 4; return c->complex_;
	case DVP_BUF_RADIUS: *bytes = L * 4; return c->radius;
	}
	*bytes = 0;
	return nullptr;
}
long long dvp_buffer_bytes(dvp_ctx* c, int id) { size_t b; buffer_ptr(c, id, &b); return (long long)b; }
// DVP_BUF_CANDIDATE is [view][pixel][8] on the device and [pixel][view][8] (the reference's order,
// main.h:41 with the view stride fixed) at the boundary
static void candidate_transpose(const dvp_ctx* c, const s2* src, s2* dst, bool to_device) {
	const size_t L = c->L, S = (size_t)c->NI - 1;
	for (size_t v = 0; v < S; ++v)
		for (size_t p = 0; p < L; ++p) {
			const size_t dev = (v * L + p) * 8, host = (p * S + v) * 8;
			std::memcpy(to_device ? dst + dev : dst + host, to_device ? src + host : src + dev, 8 * sizeof(s2));
		}
}
int dvp_download_buffer(dvp_ctx* c, int id, void* dst) {
	if (set_device(c)) return 1;
	size_t b; void* p = buffer_ptr(c, id, &b);
	if (!p) { c->error = "bad or unallocated buffer id"; return 1; }
	if (id == DVP_BUF_CANDIDATE) {
		std::vector<s2> tmp(b / sizeof(s2));
		HIP_TRY(c, hipMemcpyAsync(tmp.data(), p, b, hipMemcpyDeviceToHost, c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		candidate_transpose(c, tmp.data(), (s2*)dst, false);
		return 0;
	}
	HIP_TRY(c, hipMemcpyAsync(dst, p, b, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return 0;
}
int dvp_upload_buffer(dvp_ctx* c, int id, const void* src) {
	c->anchor_tab_valid = false;
	bump_reuse_epoch(c);
	if (set_device(c)) return 1;
	size_t b; void* p = buffer_ptr(c, id, &b);
	if (!p) { c->error = "bad or unallocated buffer id"; return 1; }
	std::vector<s2> tmp;
	if (id == DVP_BUF_CANDIDATE) {
		tmp.resize(b / sizeof(s2));
		candidate_transpose(c, (const s2*)src, tmp.data(), true);
		src = tmp.data();
	}
	HIP_TRY(c, hipMemcpyAsync(p, src, b, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return 0;
}
int dvp_weak_count(dvp_ctx* c) { return c->d.weak_count; }

int dvp_get_timings(dvp_ctx* c, DvpTimings* out) {
	if (set_device(c)) return 1;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for (auto& e : c->events) {
		float ms = 0.0f;
		HIP_TRY(c, hipEventElapsedTime(&ms, e.a, e.b));
		if (e.stage == EV_TOTAL) c->timings.total_ms += ms;
		else if (e.stage == EV_ITER_LOOP) c->timings.iter_loop_ms += ms;
		else { c->timings.stage_ms[e.stage] += ms; c->timings.stage_launches[e.stage] += 1; }
		(void)hipEventDestroy(e.a);
		(void)hipEventDestroy(e.b);
	}
	c->events.clear();
	if (out) *out = c->timings;
	return 0;
}
int dvp_reset_timings(dvp_ctx* c) {
	if (dvp_get_timings(c, nullptr)) return 1;
	std::memset(&c->timings, 0, sizeof(DvpTimings));
	return 0;
}

// ---- KAT / micro-benchmark ---------------------------------------------------------------------
int dvp_eval_cost_vectors(dvp_ctx* c, const int32_t* px, const float* planes, int n, float* out, float* kernel_ms) {
	if (set_device(c)) return 1;
	if (!c->sector_taps) { c->error = "dvp_set_params must be called first"; return 1; }
	if (n <= 0) return 0;
	const size_t S = (size_t)c->NI - 1;
	dvpmem::DevBlock dpx, dpl, dout;
	EventPairGuard ev;
	if (dpx.reserve((size_t)n * 8) || dpl.reserve((size_t)n * 16) || dout.reserve((size_t)n * S * 4)) { c->error = "dvp_eval_cost_vectors: out of device memory"; return 1; }
	HIP_TRY(c, hipMemcpyAsync(dpx.as<void>(), px, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipMemcpyAsync(dpl.as<void>(), planes, (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipEventCreate(&ev.a));
	HIP_TRY(c, hipEventCreate(&ev.b));
	HIP_TRY(c, hipEventRecord(ev.a, c->stream));
	hipLaunchKernelGGL(dvp_cost_vectors, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d, dpx.as<const int>(), dpl.as<const f4>(), n, dout.as<float>());
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(ev.b, c->stream));
	HIP_TRY(c, hipMemcpyAsync(out, dout.as<float>(), (size_t)n * S * 4, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (kernel_ms) HIP_TRY(c, hipEventElapsedTime(kernel_ms, ev.a, ev.b));
	return 0;
}

int dvp_bench_cost_kernel(dvp_ctx* c, int repeat, float* mean_kernel_ms, uint64_t* evals_per_launch) {
	if (set_device(c)) return 1;
	if (!c->sector_taps) { c->error = "dvp_set_params must be called first"; return 1; }
	if (repeat < 1) repeat = 1;
	const LaunchGeom g = make_geom(c->W, c->H, false);
	LaunchArgs a;
	a.tiles_x = g.tiles_x; a.tiles = g.tiles; a.rows = g.rows; a.half = 0; a.colour = 0; a.iter = 0;
	EventPairGuard ev;
	HIP_TRY(c, hipEventCreate(&ev.a));
	HIP_TRY(c, hipEventCreate(&ev.b));
	hipLaunchKernelGGL(dvp_cost_all_pixels, dim3(g.grid()), dim3(256), 0, c->stream, c->d, a, c->scratch_out);   // warm-up
	HIP_TRY(c, hipEventRecord(ev.a, c->stream));
	for (int i = 0; i < repeat; ++i)
		hipLaunchKernelGGL(dvp_cost_all_pixels, dim3(g.grid()), dim3(256), 0, c->stream, c->d, a, c->scratch_out);
	HIP_TRY(c, hipEventRecord(ev.b, c->stream));
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	float ms = 0.0f;
	HIP_TRY(c, hipEventElapsedTime(&ms, ev.a, ev.b));
	if (mean_kernel_ms) *mean_kernel_ms = ms / repeat;
	if (evals_per_launch) *evals_per_launch = (uint64_t)c->L * (uint64_t)(c->NI - 1);
	return 0;
}

}  // extern "C"
