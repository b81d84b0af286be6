// dvp_ctx.hpp — the engine's context and its arena: struct dvp_ctx (one HIP stream and every device buffer of one reference
// view), HIP_TRY, the arena (dalloc, dfree, alloc_group_or_fall_back: a group of optional buffers that does not fit selects a
// fall-back form), sync_dev_struct and the event-pair guard of the timed calls.  Host code only, no kernel; comes after
// dvp_kernels.hpp, whose types and using-directive it relies on.
#ifndef DVP_CTX_HPP_
#define DVP_CTX_HPP_

#include "dvp_jpeg_enc.h"
#include "dvp_edges_run.h"
#include "dvp_viewclean_run.h"
#include "dvp_prior_run.h"
#include <cstdlib>
#include <string>
#include <vector>
#include <cstdio>
#include <mutex>
#include <condition_variable>
#include <initializer_list>

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct EventPair { int stage; hipEvent_t a, b; };   // stage: launch site, or one of the two whole-run timers below
enum { EV_TOTAL = -1, EV_ITER_LOOP = -2 };

struct dvp_ctx {
	int device = 0;
	// The DVP_* switches as read when the context was created, and — the `*_fits` members below — whether the optional buffers
	// of a form could be had.  Which form a launch site takes is decided from the two by dvp_forms.hpp.
	FormSwitches sw;
	int W = 0, H = 0, NI = 0, pitch = 0;
	size_t L = 0;
	hipStream_t stream = nullptr;
	// second stream of dvp_run_patchmatch: the visibility-prior candidates (VALU-bound, read by the weak updates only)
	// run beside the latency-bound list kernels of the weak path's preparation
	// visibility-prior candidates at anchor pixels only (dvp_run_patchmatch; DVP_CAND_MASK=0: every pixel, as dvp_run_stage)
	// Which form pays depends on the WEAK share: the full launch runs on the side stream beside the latency-bound anchor search and
	// is hidden when that takes long enough (>= ~4.5 % WEAK at 6208x4128: bench cfg3, 6.9 % — masked there it would run beside
	// RandomInit and the strong update instead and cost them 28 ms); at the 1-3 % WEAK of the real schedule's full-size passes the
	// anchor search is over after 12-38 ms and the full launch was 50-60 ms exposed per view (profiles/r06_e2e_apd.txt).
	// DVP_CAND_MASK=1 / 0 forces a form; default: masked below 4 % WEAK.
	bool cand_mask_fits = true;    // false: the mark bytes did not fit
	uint8_t* cand_mask = nullptr;
	unsigned *cand_list = nullptr, *cand_n = nullptr;
	uint32_t* sel_snap = nullptr;
	hipStream_t side = nullptr;
	hipEvent_t side_fork = nullptr, side_join = nullptr;
	Dev d{};
	std::vector<void*> allocs;
	// named device buffers
	float* images = nullptr;        // row-pair planes (dvp_dev.hpp: img_texel / load_quad)
	uint8_t* images8 = nullptr;     // the same as bytes; images8_ok says whether the last upload was 8-bit exact
	int* images8_flag = nullptr;
	bool images8_ok = false;
	uint32_t* images16 = nullptr;   // the same as binary16 pairs (Dev::images16), allocated at the first upload (or dvp_ctx_reserve) that wants them
	bool images16_ok = false;       // the last upload is binary16-exact and not 8-bit exact: the weak update reads images16
	float* image_stage = nullptr;   // plain padded planes the uploads land in before dvp_interleave_rows
	float* depths = nullptr;
	uint32_t* edge_bits = nullptr;  // bit-tiled copy of `edge`, rebuilt before the launches that walk lines
	uint32_t* strong_bits = nullptr; // bit-tiled (weak_info == STRONG), rebuilt before FindNearestStrongPoint and GenNeighbours
	uint32_t* strong_bits_t = nullptr;   // ... with transposed tiles (FindNearestStrongPoint's column segments)
	int* edge_sat = nullptr;         // cell table of the edge map (Dev::edge_sat), rebuilt with edge_bits
	DvpCamera* cameras = nullptr; ViewConst* views = nullptr; int* sector_taps = nullptr; int* sector_start = nullptr;
	f4* planes = nullptr; f4* planes_snap = nullptr; f4* fit_planes = nullptr;
	int* search_pos = nullptr;   // [16][L]
	float* slot_costs = nullptr; // [17][S][half_w * H]: split strong update (allocated at its first launch)
	float* strong_rec = nullptr; // [SR_FIELDS][half_w * H]
	// plane cache of the split strong update (Dev::reuse_*), allocated with slot_costs' stand-in at the first launch
	float* reuse_costs = nullptr; PlaneKey* reuse_keys = nullptr; ReuseHdr* reuse_hdr = nullptr;
	bool reuse_fits = true;      // false: the records did not fit — the per-launch half-size cost buffer
	uint32_t reuse_epoch = 0;    // bump_reuse_epoch
	bool split_fits = true;      // false: slot_costs did not fit — the monolithic kernel
	f4* sweep_rec = nullptr; float* sweep_cost = nullptr; float* sweep_pc = nullptr;   // DepthToWeak + LocalRefine as view-compacted passes (allocated at the first fused launch)
	bool sweep_fits = true;      // false: the buffers did not fit — the fused per-pixel kernel
	int sweep_band_rows = 0;     // rows of a band of sweep_cost (DVP_SWEEP_BAND_GB; 67 GB for the whole image at 6208x4128 with 9 sources); 0 = not banded
	// the passes' evaluation launches from per-view lists (dvp_sweep_list.hpp): a group of its own, allocated behind the cost records
	uint32_t* sweep_list = nullptr; int* sweep_list_counts = nullptr;   // [S][cap] entries; [S][tiles] counts / offsets, then the lengths [S, padded to threes]
	int sweep_list_cap = 0, sweep_list_tiles = 0;   // room per view: the pixels of the image or of a band; tiles of an evaluation launch at most
	bool sweep_list_fits = true; // false: the lists did not fit — the tile form (dvp_sweep_eval)
	float* costs = nullptr; float* costs_snap = nullptr; float* complex_ = nullptr;
	uint32_t* selected_views = nullptr;
	uint8_t* view_weight = nullptr; uint8_t* weak_info = nullptr; uint8_t* weak_reliable = nullptr; uint8_t* edge = nullptr;
	s2* label_stop = nullptr; s2* weak_nearest_strong = nullptr; s2* neighbours = nullptr; s2* gn_points = nullptr; int* gn_count = nullptr; s2* candidate = nullptr; s2* edge_neigh = nullptr; s2* label_boundary = nullptr;
	int* neighbours_map = nullptr; int* label = nullptr; int* radius = nullptr;
	unsigned long long* eval_counter = nullptr;
	float* scratch_out = nullptr;
	size_t weak_alloc = 0;       // capacity (in WEAK pixels) of the per-WEAK buffers
	AnchorRec* anchor_tab = nullptr;   // [WEAK][S][11] reference sides of the anchor sub-patches (dvp_weak_wave.hpp), allocated at the first weak update
	size_t anchor_tab_alloc = 0;       // capacity in records
	bool anchor_tab_valid = false;     // built for the current anchors / offsets / images (any launch or upload that can change them clears it)
	bool anchor_tab_fits = true;       // false: the table did not fit — the weak update forms the reference side per item
	// the weak update as seven launches (dvp_weak_phased.hpp): per-WEAK-pixel hand-over, allocated at the first weak update
	WeakRec* weak_rec = nullptr; f2* weak_ctab = nullptr; float* weak_ev = nullptr;
	size_t weak_phase_alloc = 0;       // capacity in WEAK pixels
	bool weak_phase_fits = true;       // false: the buffers did not fit — the one-wave form
	int* weak_list = nullptr;    // compacted WEAK pixel indices (black first, then red)
	size_t weak_list_alloc = 0;
	int* weak_counts = nullptr;  // scratch of the device-side compaction: per-slot black / red counts, per-chunk counts, then 3 totals
	int* weak_totals_host = nullptr;   // pinned: (black, red, all)
	uint8_t* coarse = nullptr;   // staging of the coarser level's maps (dvp_upload_state_rescaled)
	uint8_t* maps_out = nullptr; // staging of dvp_download_maps: depth [L] f32, normal [L][3] f32, selected views [L] u32, radius [L] i32, states [L] u8 (words first: all aligned)
	// dvp_download_maps_begin / _finish: the copies to the host run on their own stream, from any thread, while this context is
	// already on its next view; `dl_busy` = maps_out holds maps that have not been fetched yet
	hipStream_t copy = nullptr;
	uint8_t* maps_host = nullptr;   // pinned mirror of maps_out (one DMA, no staging through the runtime's pageable-copy path)
	std::mutex dl_m;
	std::condition_variable dl_cv;
	bool dl_busy = false;
	bool dl_fetching = false;   // a dvp_download_maps_finish call is running right now (it ends in bounded time)
	size_t coarse_alloc = 0;
	// dvp_preview_begin / _finish: the rendered previews (BGR) and their encodes, one slot per kind; like maps_out they are
	// overwritten by the next dvp_preview_begin only
	uint8_t* pv_bgr[3] = { nullptr, nullptr, nullptr };
	dvpjpeg::Encoder pv_enc[3];
	unsigned long long* pv_total = nullptr;   // pinned: the encodes' data sizes
	hipEvent_t pv_done = nullptr;             // the last dvp_preview_begin's work on `stream`
	hipStream_t pv_copy = nullptr;            // the fetches of dvp_preview_finish / _pixels (any thread)
	int pv_kinds = 0;
	// dvp_edge_map_begin / _finish: the Canny edge prior from image 0 (dvp_edges.hip).  Scratch and output maps exist from the
	// first dvp_edge_map_begin (or dvp_ctx_reserve bit 3) on.  Two output slots: a driver fetches a view's map in the view's
	// background job, when the context may have begun the next view's map already; _finish serves begun maps oldest first, and
	// a third _begin overwrites the oldest map nobody fetched.
	dvpedge::Scratch eg;
	struct EdgeSlot { dvpmem::DevBlock map; hipEvent_t done = nullptr; unsigned long long seq = 0; bool pending = false, fetching = false; };
	EdgeSlot eg_slot[2];
	unsigned long long eg_seq = 0;
	hipStream_t eg_copy = nullptr;            // the fetches of dvp_edge_map_finish (any thread)
	std::mutex eg_m;
	std::condition_variable eg_cv;
	bool have_images = false;                 // dvp_upload_images* has run
	// dvp_set_view_cleanup: the visibility-mask clean-up of the staged selected-view words (dvp_viewclean.hip).  The scratch exists
	// from the first dvp_download_maps_begin with the clean-up on (or dvp_ctx_reserve bit 4) on.
	dvpvc::Scratch vc;
	bool vc_on = false;
	int vc_num_src = 0, vc_min_region = 0;
	// dvp_plane_prior: the monocular-depth plane prior of a FIRST_INIT pass (dvp_prior.hip).  The scratch exists from the first call on.
	dvpprior::Scratch pr;
	bool have_cameras = false;                // dvp_upload_cameras has run
	// dvp_save_state / dvp_restore_state: device-side copy of the per-pixel input state
	f4* saved_planes = nullptr; uint32_t* saved_views = nullptr; uint8_t* saved_weak = nullptr; int* saved_radius = nullptr;
	bool have_saved = false;
	int lut_radius = -1;
	bool have_depths = false;
	bool profiling = false;
	std::vector<EventPair> events;
	DvpTimings timings{};
	std::string error;
};

static std::string g_create_error;

#define HIP_TRY(ctx, expr)                                                                          \
	do {                                                                                            \
		hipError_t e_ = (expr);                                                                     \
		if (e_ != hipSuccess) {                                                                     \
			char buf_[512];                                                                         \
			snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			(ctx)->error = buf_;                                                                    \
			return 1;                                                                               \
		}                                                                                           \
	} while (0)

template <class T>
static int dalloc(dvp_ctx* c, T** p, size_t count, bool zero = true) {
	void* q = nullptr;
	const size_t bytes = (count ? count : 1) * sizeof(T);
	HIP_TRY(c, hipMalloc(&q, bytes));
	c->allocs.push_back(q);
	if (zero) HIP_TRY(c, hipMemsetAsync(q, 0, bytes, c->stream));
	*p = (T*)q;
	return 0;
}

// give a superseded block back (the caller has made sure no queued work still uses it)
template <class T>
static void dfree(dvp_ctx* c, T** p) {
	if (!*p) return;
	for (size_t i = 0; i < c->allocs.size(); ++i)
		if (c->allocs[i] == (void*)*p) { c->allocs[i] = c->allocs.back(); c->allocs.pop_back(); break; }
	(void)hipFree((void*)*p);
	*p = nullptr;
}

// one block of a group of optional buffers (alloc_group_or_fall_back)
struct AllocReq { void** p; size_t bytes; bool zero; };   // p == nullptr: nothing to allocate
template <class T>
static AllocReq areq(T** p, size_t bytes, bool zero = false) { return { reinterpret_cast<void**>(p), bytes, zero }; }

// The plane cache's records (Dev::reuse_*) hold cost vectors from one strong update of a pass to the next.  A vector depends on
// the images, the cameras, the parameters, the sampler and the radius map (the header checks the pixel's own radius): every call
// that can change one of them, and the start of every dvp_run_patchmatch, makes all records empty by moving on to a new epoch.
static void bump_reuse_epoch(dvp_ctx* c) {
	if (++c->reuse_epoch == 0) {   // wrapped: headers of 2^32 epochs ago must not match
		if (c->reuse_hdr) (void)hipMemsetAsync(c->reuse_hdr, 0, c->L * sizeof(ReuseHdr), c->stream);
		c->reuse_epoch = 1;
	}
	c->d.reuse_epoch = c->reuse_epoch;
}

static size_t img16_plane_bytes(int W, int H) { return (size_t)img16_tiles_x(W) * img16_tiles_y(H) * 128; }

static bool anchor_table_off(const dvp_ctx* c) { return c->sw.anchor_tab_off || !c->anchor_tab_fits; }

static void sync_dev_struct(dvp_ctx* c) {
	Dev& d = c->d;
	d.width = c->W; d.height = c->H; d.num_images = c->NI; d.pitch = c->pitch;
	d.org = kImgPad * c->pitch + kImgPad;
	d.plane_stride = (size_t)c->pitch * (c->H + 2 * kImgPad);
	d.images = c->images; d.images8 = c->images8_ok ? c->images8 : nullptr; d.img8_tiles_x = img8_tiles_x(c->W); d.img8_plane_bytes = (size_t)img8_tiles_x(c->W) * img8_tiles_y(c->H) * 128;
	d.images16 = c->images16_ok ? c->images16 : nullptr; d.img16_tiles_x = img16_tiles_x(c->W); d.img16_plane_bytes = img16_plane_bytes(c->W, c->H);
	d.depths = c->depths; d.cameras = c->cameras; d.views = c->views; d.sector_taps = c->sector_taps; d.sector_start = c->sector_start;
	d.search_pos = c->search_pos;
	d.sweep_px0 = 0; d.sweep_row0 = 0; d.sweep_row1 = 0;   // (set per band by the sweep passes' launches)
	d.sweep_all_slots = c->sw.sweep_all_slots ? 1 : 0;
	d.sweep_rec = c->sweep_rec; d.sweep_cost = c->sweep_cost; d.sweep_pc = c->sweep_pc; d.slot_costs = c->slot_costs; d.strong_rec = c->strong_rec; d.half_w = (c->W + 1) / 2;
	d.sweep_list = c->sweep_list; d.sweep_list_counts = c->sweep_list_counts; d.sweep_list_cap = c->sweep_list_cap;
	d.sweep_list_n = c->sweep_list_counts ? c->sweep_list_counts + (size_t)(c->NI - 1) * c->sweep_list_tiles : nullptr;
	d.reuse_costs = c->reuse_costs; d.reuse_keys = c->reuse_keys; d.reuse_hdr = c->reuse_hdr; d.reuse_epoch = c->reuse_epoch;
	d.planes = c->planes; d.planes_snap = c->planes_snap; d.costs = c->costs; d.costs_snap = c->costs_snap;
	d.selected_views = c->selected_views; d.view_weight = c->view_weight; d.weak_info = c->weak_info;
	d.weak_reliable = c->weak_reliable; d.weak_nearest_strong = c->weak_nearest_strong;
	d.anchor_tab = (anchor_table_off(c) || !c->anchor_tab_valid) ? nullptr : c->anchor_tab; d.neighbours_map = c->neighbours_map; d.neighbours = c->neighbours; d.gn_points = c->gn_points; d.gn_count = c->gn_count; d.fit_planes = c->fit_planes;
	d.candidate = c->candidate; d.edge = c->edge; d.edge_bits = c->edge_bits; d.strong_bits = c->strong_bits; d.strong_bits_t = c->strong_bits_t; d.edge_sat = c->edge_sat; d.sat_cells_x = sat_cells(c->W); d.sat_cells_y = sat_cells(c->H); d.edge_tiles_x = edge_tiles_x(c->W); d.edge_neigh = c->edge_neigh; d.label = c->label;
	d.label_boundary = c->label_boundary; d.label_stop = c->label_stop; d.complex_ = c->complex_; d.radius = c->radius;
	d.weak_list = c->weak_list;
	d.weak_rec = c->weak_rec; d.weak_ctab = c->weak_ctab; d.weak_ev = c->weak_ev;
	d.eval_counter = c->profiling ? c->eval_counter : nullptr;
}

// the binary16 planes, allocated once per context and only by the contexts that see such image sets (or are told to expect them)
static int ensure_images16(dvp_ctx* c) {
	if (c->images16) return 0;
	return dalloc(c, &c->images16, img16_plane_bytes(c->W, c->H) / 4 * c->NI, false);
}

static int set_device(dvp_ctx* c) {
	HIP_TRY(c, hipSetDevice(c->device));
	return 0;
}

// All of `reqs` (four at most), in order, or none of them.  On success the pointers are set, owned by the context and in c->d.
// Otherwise *fits goes false and `msg`, a format with one %f for `gb`, says so.  `hook`: the tests' environment variable that
// takes the fall-back without trying.  `retry_bytes`: a smaller size to try for the first block when the asked one is refused.
// Returns the bytes of the first block, 0 for the fall-back.
static size_t alloc_group_or_fall_back(dvp_ctx* c, std::initializer_list<AllocReq> reqs, const char* hook, bool* fits, const char* msg, double gb, size_t retry_bytes = 0) {
	void* got[4] = { nullptr, nullptr, nullptr, nullptr };
	const AllocReq* r = reqs.begin();
	const size_t n = reqs.size();
	size_t first = r[0].bytes;
	bool ok = n <= 4 && !(hook && getenv(hook));
	for (size_t i = 0; i < n && ok; ++i) {
		if (!r[i].p) continue;
		ok = hipMalloc(&got[i], r[i].bytes) == hipSuccess;
		if (!ok && i == 0 && retry_bytes) { (void)hipGetLastError(); first = retry_bytes; ok = hipMalloc(&got[0], first) == hipSuccess; }
		if (!ok) got[i] = nullptr;
		else if (r[i].zero) ok = hipMemsetAsync(got[i], 0, r[i].bytes, c->stream) == hipSuccess;   // (never the block with a retry size)
	}
	if (!ok) {
		(void)hipGetLastError();   // clear the sticky out-of-memory status
		for (void* q : got) if (q) (void)hipFree(q);
		*fits = false;
		if (msg) fprintf(stderr, msg, gb);
	}
	else for (size_t i = 0; i < n; ++i) if (r[i].p) { *r[i].p = got[i]; c->allocs.push_back(got[i]); }
	sync_dev_struct(c);   // (also after a refusal: the callers have freed the blocks they were replacing)
	return ok ? first : 0;
}

namespace {
struct EventPairGuard {
	hipEvent_t a = nullptr, b = nullptr;
	~EventPairGuard() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};
}  // namespace

#endif
