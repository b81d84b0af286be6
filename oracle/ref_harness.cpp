// REFERENCE PIN — TEST INFRASTRUCTURE ONLY.
// Host harness around the reference's own device text (the part of APD.cu in front of
// APD::RunPatchMatch, cut and compiled by make_ref.py against oracle/ref_shim/).  It offers the C ABI
// of ora_api.cpp — same stage and buffer ids — so that tests/test_reference_pin.py can put the
// oracle's pre-launch state into it, run one launch in both and compare every buffer.
//
// A launch here is, as in the oracle, the per-pixel function of the pre-launch state: every thread of
// the launch geometry (restated from APD.cu:4409-4428) runs on the live arrays, the rows its pixel owns
// are copied out, and the pre-launch values are put back before the next thread.  The rows a pixel
// owns are its pixel-indexed entries and, for a WEAK pixel, row neighbours_map[pixel] of the
// WEAK-indexed buffers.  ref_set_debug(1) compares the whole state (guard bands included) with the
// snapshot after every thread and records the first pixel that wrote outside its own rows.
//
// Buffers are sized as APD::CudaSpaceInitialization sizes them (APD.cpp:1552-1605), candidate_cuda
// with the reference's own stride of NUM_IMAGES = 4 views (main.h:41, APD.cpp:1573).  That stride
// aliases for more than four source views, so candidate get/set (oracle layout [pixel][S][8]) is
// refused for S > 4.  The reference reads a little outside some buffers (selected_views one row past
// the end, APD.cu:2473; the edge map in BresenhamLine, APD.cu:267-311): every buffer has a zeroed
// guard band in front and behind.
// ora_common.h first: its constants (namespace ora) carry the names main.h defines as macros
#include "ora_common.h"       // ours: the counter-based generator and its site keys, namespace ora
#include "APD.h"              // the reference's, from the cut folder (DataPassHelper, Camera, params)
#include <vector>

uint3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
int dvp_ref_sampler = 0;

// ---- the device text's entry points (declarations restated; definitions in the cut text) ----------
void GenEdgeInform(DataPassHelper*);
void FindNearestStrongPoint(DataPassHelper*);
void GenNeighbours(DataPassHelper*);
void NeigbourUpdate(DataPassHelper*);
void RandomInitialization(DataPassHelper*);
void BlackPixelUpdateStrong(const int, DataPassHelper*);
void RedPixelUpdateStrong(const int, DataPassHelper*);
void RANSACToGetFitPlane(DataPassHelper*);
void BlackPixelUpdateWeak(const int, DataPassHelper*);
void RedPixelUpdateWeak(const int, DataPassHelper*);
void GetDepthandNormal(DataPassHelper*);
void BlackPixelFilterStrong(DataPassHelper*);
void RedPixelFilterStrong(DataPassHelper*);
void DepthToWeak(DataPassHelper*);
void LocalRefine(DataPassHelper*);
void ComputeHomography(const Camera, const Camera, const float4, float*);
float2 ComputeCorrespondingPoint(const float*, const int2);
float ComputeBilateralNCCOld(const int2, const int, const float4, const DataPassHelper*);
float ComputeBilateralNCCNew(const int2, const int, const float4, const DataPassHelper*);
float ComputeGeomConsistencyCost(const int2, const int, const float4, DataPassHelper*);
void ComputeMultiViewCostVectorOld(const int2, float4, float*, DataPassHelper*);
bool BresenhamLine(int2, int2, const DataPassHelper*);
bool PointinTriangle(short2, short2, short2, int2);

static_assert(sizeof(Camera) == sizeof(ora::Camera), "Camera layout");
static_assert(sizeof(PatchMatchParams) == sizeof(ora::PatchMatchParams), "PatchMatchParams layout");

namespace {

enum Stage {   // == OraStage (ora_api.cpp)
	ST_GEN_EDGE_INFORM = 0, ST_FIND_NEAREST_STRONG = 1, ST_GEN_NEIGHBOURS = 2, ST_NEIGHBOUR_UPDATE = 3,
	ST_RANDOM_INIT = 4, ST_STRONG_UPDATE = 5, ST_RANSAC_FIT = 6, ST_WEAK_UPDATE = 7,
	ST_GET_DEPTH_NORMAL = 8, ST_FILTER_STRONG = 9, ST_DEPTH_TO_WEAK = 10, ST_LOCAL_REFINE = 11,
};
enum Buffer {  // == OraBuffer (ora_api.cpp)
	BUF_PLANES = 0, BUF_COSTS = 1, BUF_SELECTED_VIEWS = 2, BUF_VIEW_WEIGHT = 3, BUF_WEAK_INFO = 4,
	BUF_WEAK_RELIABLE = 5, BUF_WEAK_NEAREST_STRONG = 6, BUF_NEIGHBOURS_MAP = 7, BUF_NEIGHBOURS = 8,
	BUF_FIT_PLANES = 9, BUF_CANDIDATE = 10, BUF_EDGE = 11, BUF_EDGE_NEIGH = 12, BUF_LABEL = 13,
	BUF_LABEL_BOUNDARY = 14, BUF_COMPLEX = 15, BUF_RADIUS = 16, BUF_COUNT = 17,
};

// one state buffer: `rows` rows of `row_bytes`, with a zeroed guard band on both sides
struct Buf {
	std::vector<unsigned char> store;
	size_t row_bytes = 0, rows = 0, guard = 0;
	bool per_weak = false;   // indexed by neighbours_map[pixel] (WEAK pixels only) instead of by pixel
	void init(size_t rows_, size_t row_bytes_, size_t guard_rows, bool per_weak_, int fill) {
		rows = rows_; row_bytes = row_bytes_; per_weak = per_weak_;
		guard = guard_rows * row_bytes;
		store.assign(2 * guard + rows * row_bytes, 0);
		if (fill) std::memset(data(), fill, rows * row_bytes);
	}
	unsigned char* data() { return store.data() + guard; }
	size_t bytes() const { return rows * row_bytes; }
};

struct Ref {
	int width = 0, height = 0, num_images = 0, sampler = 0, debug = 0;
	uint64_t seed = 0;
	int weak_count = 0;
	PatchMatchParams params;
	Camera cameras[MAX_IMAGES];
	std::vector<float> images[MAX_IMAGES], depths[MAX_IMAGES];
	RefTexture image_tex[MAX_IMAGES], depth_tex[MAX_IMAGES];
	cudaTextureObjects image_objs, depth_objs;
	std::vector<curandState> rand_states;
	Buf buf[BUF_COUNT];
	DataPassHelper helper;
	// outcome of the last launch
	int bad_line = 0;                 // a draw from a source line the table does not know
	int viol_pixel = -1, viol_buf = -1;   // debug: first thread that wrote outside its pixel's rows
	long long viol_count = 0;
};

// ---- draws ------------------------------------------------------------------------------------------
// ref_draws.inc is generated by make_ref.py from oracle/ref_draws.json: {first line, last line, sub}.
// sub >= 0 is an ora::RngSub; DRAW_DISCARD marks draws whose values cannot reach any output.
const int DRAW_DISCARD = -1;
struct DrawRange { int first, last, sub; };
const DrawRange kDraws[] = {
#include "ref_draws.inc"
};
struct DrawState {
	Ref* ctx = nullptr;
	int phase = 0, iter = 0, pixel = -1;
	uint32_t k[8] = {0};
} g_draw;

int draw_sub(int line) {
	for (const DrawRange& r : kDraws)
		if (line >= r.first && line <= r.last) return r.sub;
	if (g_draw.ctx && !g_draw.ctx->bad_line) g_draw.ctx->bad_line = line;
	return -2;
}
uint32_t draw_site(int sub) { return ora::rng_site(g_draw.phase, g_draw.iter, sub); }
bool draw_ok() {
	if (g_draw.phase > 0 && g_draw.pixel >= 0) return true;
	if (g_draw.ctx && !g_draw.ctx->bad_line) g_draw.ctx->bad_line = -1;   // a draw in a launch that has none
	return false;
}

void reset_draws(Ref& h, int phase, int iter, int pixel) {
	g_draw.ctx = &h; g_draw.phase = phase; g_draw.iter = iter; g_draw.pixel = pixel;
	std::memset(g_draw.k, 0, sizeof(g_draw.k));
}

void alloc_state(Ref& h) {
	const size_t L = (size_t)h.width * h.height;
	const size_t g = 2 * (size_t)h.width + 64;   // guard rows
	h.buf[BUF_PLANES].init(L, sizeof(float4), g, false, 0);
	h.buf[BUF_COSTS].init(L, 4, g, false, 0);
	h.buf[BUF_SELECTED_VIEWS].init(L, 4, g, false, 0);
	h.buf[BUF_VIEW_WEIGHT].init(L, MAX_IMAGES, g, false, 0);
	h.buf[BUF_WEAK_INFO].init(L, 1, g, false, 0);
	std::memset(h.buf[BUF_WEAK_INFO].data(), STRONG, L);
	h.buf[BUF_WEAK_RELIABLE].init(L, 1, g, false, 0);
	h.buf[BUF_WEAK_NEAREST_STRONG].init(L, sizeof(short2), g, false, 0xff);
	h.buf[BUF_NEIGHBOURS_MAP].init(L, 4, g, false, 0);
	h.buf[BUF_FIT_PLANES].init(L, sizeof(float4), g, false, 0);                              // APD.cpp:1570-1571
	h.buf[BUF_CANDIDATE].init(L, LAB_BOUNDARY_NUM * NUM_IMAGES * sizeof(short2), g, false, 0);   // APD.cpp:1573
	h.buf[BUF_EDGE].init(L, 1, g, false, 0);
	h.buf[BUF_EDGE_NEIGH].init(L, EDGE_NEIGH_NUM * sizeof(short2), g, false, 0xff);          // APD.cpp:1581
	h.buf[BUF_LABEL].init(L, 4, g, false, 0);
	h.buf[BUF_RADIUS].init(L, 4, g, false, 0);
	int* radius = (int*)h.buf[BUF_RADIUS].data();
	for (size_t i = 0; i < L; ++i) radius[i] = 5;
	h.rand_states.assign(L, curandState{0});
}

void alloc_weak(Ref& h) {   // APD.cpp:1582, 1587, 1605: one row per WEAK pixel
	const size_t wc = (size_t)(h.weak_count > 0 ? h.weak_count : 1);
	h.buf[BUF_NEIGHBOURS].init(wc, NEIGHBOUR_NUM * sizeof(short2), 64, true, 0xff);
	h.buf[BUF_LABEL_BOUNDARY].init(wc, LAB_BOUNDARY_NUM * sizeof(short2), 64, true, 0xff);
	h.buf[BUF_COMPLEX].init(wc, 4, 64, true, 0);
}

void fill_helper(Ref& h) {   // APD::SetDataPassHelperInCuda
	for (int i = 0; i < h.num_images; ++i) {
		h.image_tex[i] = RefTexture{h.images[i].data(), h.width, h.height};
		h.depth_tex[i] = RefTexture{h.depths[i].data(), h.width, h.height};
		h.image_objs.images[i] = (cudaTextureObject_t)(uintptr_t)&h.image_tex[i];
		h.depth_objs.images[i] = (cudaTextureObject_t)(uintptr_t)&h.depth_tex[i];
	}
	DataPassHelper& d = h.helper;
	std::memset(&d, 0, sizeof(d));
	d.width = h.width;
	d.height = h.height;
	d.ref_index = 0;
	d.texture_objects_cuda = &h.image_objs;
	d.texture_depths_cuda = &h.depth_objs;
	d.cameras_cuda = h.cameras;
	d.plane_hypotheses_cuda = (float4*)h.buf[BUF_PLANES].data();
	d.rand_states_cuda = h.rand_states.data();
	d.selected_views_cuda = (unsigned int*)h.buf[BUF_SELECTED_VIEWS].data();
	d.neighbours_cuda = (short2*)h.buf[BUF_NEIGHBOURS].data();
	d.neighbours_map_cuda = (int*)h.buf[BUF_NEIGHBOURS_MAP].data();
	d.weak_info_cuda = h.buf[BUF_WEAK_INFO].data();
	d.costs_cuda = (float*)h.buf[BUF_COSTS].data();
	d.params = &h.params;
	d.debug_point = make_int2(-1000, -1000);   // outside any image
	d.show_ncc_info = false;
	d.fit_plane_hypotheses_cuda = (float4*)h.buf[BUF_FIT_PLANES].data();
	d.label_cuda = (int*)h.buf[BUF_LABEL].data();
	d.label_boundary_cuda = (short2*)h.buf[BUF_LABEL_BOUNDARY].data();
	d.candidate_cuda = (short2*)h.buf[BUF_CANDIDATE].data();
	d.weak_reliable_cuda = h.buf[BUF_WEAK_RELIABLE].data();
	d.view_weight_cuda = h.buf[BUF_VIEW_WEIGHT].data();
	d.weak_nearest_strong = (short2*)h.buf[BUF_WEAK_NEAREST_STRONG].data();
	d.edge_cuda = h.buf[BUF_EDGE].data();
	d.edge_neigh_cuda = (short2*)h.buf[BUF_EDGE_NEIGH].data();
	d.complex_cuda = (float*)h.buf[BUF_COMPLEX].data();
	d.radius_cuda = (int*)h.buf[BUF_RADIUS].data();
	dvp_ref_sampler = h.sampler;
}

void run_thread(Ref& h, int stage, int iter, int colour) {
	DataPassHelper* d = &h.helper;
	switch (stage) {
	case ST_GEN_EDGE_INFORM: GenEdgeInform(d); break;
	case ST_FIND_NEAREST_STRONG: FindNearestStrongPoint(d); break;
	case ST_GEN_NEIGHBOURS: GenNeighbours(d); break;
	case ST_NEIGHBOUR_UPDATE: NeigbourUpdate(d); break;
	case ST_RANDOM_INIT: RandomInitialization(d); break;
	case ST_STRONG_UPDATE: if (colour) RedPixelUpdateStrong(iter, d); else BlackPixelUpdateStrong(iter, d); break;
	case ST_RANSAC_FIT: RANSACToGetFitPlane(d); break;
	case ST_WEAK_UPDATE: if (colour) RedPixelUpdateWeak(iter, d); else BlackPixelUpdateWeak(iter, d); break;
	case ST_GET_DEPTH_NORMAL: GetDepthandNormal(d); break;
	case ST_FILTER_STRONG: if (colour) RedPixelFilterStrong(d); else BlackPixelFilterStrong(d); break;
	case ST_DEPTH_TO_WEAK: DepthToWeak(d); break;
	case ST_LOCAL_REFINE: LocalRefine(d); break;
	}
}

}  // namespace

float dvp_ref_uniform(int line) {
	const int sub = draw_sub(line);
	if (sub == DRAW_DISCARD) return 0.5f;
	if (sub < 0 || !draw_ok()) return 0.5f;
	return ora::dvp_rand_uniform(g_draw.ctx->seed, (uint32_t)g_draw.pixel, draw_site(sub), g_draw.k[sub]++);
}
unsigned dvp_ref_u32(int line) {
	const int sub = draw_sub(line);
	if (sub < 0 || !draw_ok()) return 0u;
	return ora::dvp_rand_u32(g_draw.ctx->seed, (uint32_t)g_draw.pixel, draw_site(sub), g_draw.k[sub]++);
}

extern "C" {

void* ref_create(int width, int height, int num_images) {
	if (num_images < 1 || num_images > MAX_IMAGES) return nullptr;
	Ref* h = new Ref();
	h->width = width; h->height = height; h->num_images = num_images;
	std::memset(h->cameras, 0, sizeof(h->cameras));
	std::memset((void*)&h->params, 0, sizeof(h->params));
	for (int i = 0; i < num_images; ++i) {
		h->images[i].assign((size_t)width * height, 0.0f);
		h->depths[i].assign((size_t)width * height, 0.0f);
	}
	alloc_state(*h);
	alloc_weak(*h);
	return h;
}
void ref_destroy(void* c) { delete (Ref*)c; }
void ref_set_image(void* c, int idx, const float* data) { Ref& h = *(Ref*)c; h.images[idx].assign(data, data + (size_t)h.width * h.height); }
void ref_set_depth(void* c, int idx, const float* data) { Ref& h = *(Ref*)c; h.depths[idx].assign(data, data + (size_t)h.width * h.height); }
void ref_set_cameras(void* c, const Camera* cams, int n) { Ref& h = *(Ref*)c; for (int i = 0; i < n; ++i) h.cameras[i] = cams[i]; }
void ref_set_params(void* c, const void* p) { std::memcpy((void*)&((Ref*)c)->params, p, sizeof(PatchMatchParams)); }
void ref_set_seed(void* c, uint64_t seed) { ((Ref*)c)->seed = seed; }
void ref_set_sampler(void* c, int sampler) { ((Ref*)c)->sampler = sampler; }
void ref_set_debug(void* c, int on) { ((Ref*)c)->debug = on; }
int ref_weak_count(void* c) { return ((Ref*)c)->weak_count; }
int ref_draw_ranges(void) { return (int)(sizeof(kDraws) / sizeof(kDraws[0])); }

// same meaning as ora_upload_state: any pointer may be null; weak_info also rebuilds neighbours_map /
// weak_count (APD.cpp:1182-1193) and re-sizes the WEAK-indexed buffers.
void ref_upload_state(void* c, const float4* planes, const uint32_t* views, const uint8_t* weak,
	const uint8_t* edge, const int* label, const int* radius) {
	Ref& h = *(Ref*)c;
	const size_t L = (size_t)h.width * h.height;
	if (planes) std::memcpy(h.buf[BUF_PLANES].data(), planes, L * sizeof(float4));
	if (views) std::memcpy(h.buf[BUF_SELECTED_VIEWS].data(), views, L * 4);
	if (edge) std::memcpy(h.buf[BUF_EDGE].data(), edge, L);
	if (label) std::memcpy(h.buf[BUF_LABEL].data(), label, L * 4);
	if (radius) std::memcpy(h.buf[BUF_RADIUS].data(), radius, L * 4);
	if (weak) std::memcpy(h.buf[BUF_WEAK_INFO].data(), weak, L);
	const uint8_t* wi = h.buf[BUF_WEAK_INFO].data();
	int* map = (int*)h.buf[BUF_NEIGHBOURS_MAP].data();
	h.weak_count = 0;
	for (size_t i = 0; i < L; ++i) {
		map[i] = 0;
		if (wi[i] == WEAK) map[i] = h.weak_count++;
	}
	alloc_weak(h);
}

long long ref_buffer_bytes(void* c, int id) {
	Ref& h = *(Ref*)c;
	if (id < 0 || id >= BUF_COUNT) return 0;
	if (id == BUF_CANDIDATE) {
		const int S = h.num_images - 1;
		return (long long)h.width * h.height * (S > 0 ? S : 1) * LAB_BOUNDARY_NUM * (long long)sizeof(short2);
	}
	return (long long)h.buf[id].bytes();
}
// candidate crosses between the oracle's layout [pixel][S][8] and the reference's [pixel][4][8]
static int candidate_copy(Ref& h, void* ext, bool to_ext) {
	const int S = h.num_images - 1;
	if (S > NUM_IMAGES) return -2;
	const size_t L = (size_t)h.width * h.height, row = LAB_BOUNDARY_NUM * sizeof(short2);
	unsigned char* in = h.buf[BUF_CANDIDATE].data();
	for (size_t p = 0; p < L; ++p)
		for (int v = 0; v < S; ++v) {
			unsigned char* a = (unsigned char*)ext + (p * S + v) * row;
			unsigned char* b = in + (p * NUM_IMAGES + v) * row;
			if (to_ext) std::memcpy(a, b, row); else std::memcpy(b, a, row);
		}
	return 0;
}
int ref_get_buffer(void* c, int id, void* dst) {
	Ref& h = *(Ref*)c;
	if (id < 0 || id >= BUF_COUNT) return -1;
	if (id == BUF_CANDIDATE) return candidate_copy(h, dst, true);
	std::memcpy(dst, h.buf[id].data(), h.buf[id].bytes());
	return 0;
}
int ref_set_buffer(void* c, int id, const void* src) {
	Ref& h = *(Ref*)c;
	if (id < 0 || id >= BUF_COUNT) return -1;
	if (id == BUF_CANDIDATE) return candidate_copy(h, (void*)src, false);
	std::memcpy(h.buf[id].data(), src, h.buf[id].bytes());
	return 0;
}

// One kernel launch of APD.cu:4430-4505.  Returns 0, -1 for an unknown stage, -2 for a draw the table
// cannot key (ref_last_bad_line tells the source line; -1 there: a draw in a launch the oracle has
// none in).  Ownership violations do not fail the launch: ask ref_violation.
int ref_run_stage(void* c, int stage, int iter, int colour) {
	Ref& h = *(Ref*)c;
	if (stage < ST_GEN_EDGE_INFORM || stage > ST_LOCAL_REFINE) return -1;
	fill_helper(h);
	h.bad_line = 0; h.viol_pixel = -1; h.viol_buf = -1; h.viol_count = 0;
	const int W = h.width, H = h.height;
	const bool half = stage == ST_STRONG_UPDATE || stage == ST_WEAK_UPDATE || stage == ST_FILTER_STRONG;
	int phase = 0, rng_iter = 0;
	switch (stage) {   // where the oracle constructs its Rng objects (ora_kernels.cpp, ora_weak.cpp)
	case ST_RANDOM_INIT: phase = ora::PH_RANDOM_INIT; break;
	case ST_STRONG_UPDATE: phase = ora::PH_STRONG; rng_iter = iter; break;
	case ST_RANSAC_FIT: phase = ora::PH_RANSAC; rng_iter = iter; break;
	case ST_WEAK_UPDATE: phase = ora::PH_WEAK; rng_iter = iter; break;
	case ST_GEN_NEIGHBOURS: phase = ora::PH_NEIGHBOURS; break;
	}
	// launch geometry, APD.cu:4409-4428
	if (half) {
		blockDim.x = 32; blockDim.y = 16;
		gridDim.x = (W + 32 - 1) / 32; gridDim.y = ((H / 2) + 16 - 1) / 16;
	} else {
		blockDim.x = 16; blockDim.y = 16;
		gridDim.x = (W + 16 - 1) / 16; gridDim.y = (H + 16 - 1) / 16;
	}
	blockDim.z = gridDim.z = 1;
	threadIdx.z = blockIdx.z = 0;

	std::vector<unsigned char> pre[BUF_COUNT], out[BUF_COUNT];
	for (int b = 0; b < BUF_COUNT; ++b) { pre[b] = h.buf[b].store; out[b] = h.buf[b].store; }
	const std::vector<unsigned char>& pre_weak = pre[BUF_WEAK_INFO];
	const std::vector<unsigned char>& pre_map = pre[BUF_NEIGHBOURS_MAP];

	for (unsigned by = 0; by < gridDim.y; ++by)
	for (unsigned bx = 0; bx < gridDim.x; ++bx)
	for (unsigned ty = 0; ty < blockDim.y; ++ty)
	for (unsigned tx = 0; tx < blockDim.x; ++tx) {
		blockIdx.x = bx; blockIdx.y = by; threadIdx.x = tx; threadIdx.y = ty;
		// the pixel this thread works on: the kernels' own map (APD.cu:3093-3100 for the half launches)
		int px = (int)(bx * blockDim.x + tx), py = (int)(by * blockDim.y + ty);
		if (half) py = 2 * py + (int)((tx & 1u) ^ (unsigned)colour);
		const int pixel = (px < W && py < H) ? px + py * W : -1;
		reset_draws(h, phase, rng_iter, pixel);
		run_thread(h, stage, iter, colour);
		// copy out the rows the pixel owns, then put the pre-launch values back
		for (int b = 0; b < BUF_COUNT; ++b) {
			Buf& u = h.buf[b];
			long long row = -1;
			if (pixel >= 0) {
				if (!u.per_weak) row = pixel;
				else if (pre_weak[h.buf[BUF_WEAK_INFO].guard + pixel] == WEAK) {
					int m;
					std::memcpy(&m, &pre_map[h.buf[BUF_NEIGHBOURS_MAP].guard + (size_t)pixel * 4], 4);
					if (m >= 0 && (size_t)m < u.rows) row = m;
				}
			}
			if (row >= 0) {
				const size_t off = u.guard + (size_t)row * u.row_bytes;
				std::memcpy(&out[b][off], &u.store[off], u.row_bytes);
				std::memcpy(&u.store[off], &pre[b][off], u.row_bytes);
			}
			if (h.debug && std::memcmp(u.store.data(), pre[b].data(), u.store.size()) != 0) {
				if (h.viol_count++ == 0) { h.viol_pixel = pixel; h.viol_buf = b; }
				u.store = pre[b];
			}
		}
	}
	for (int b = 0; b < BUF_COUNT; ++b) h.buf[b].store.swap(out[b]);
	g_draw.ctx = nullptr;
	return h.bad_line ? -2 : 0;
}
int ref_last_bad_line(void* c) { return ((Ref*)c)->bad_line; }
// debug switch only: number of threads that wrote outside their pixel's rows in the last launch; the
// first one's pixel and buffer id through the pointers
long long ref_violation(void* c, int* pixel, int* buffer) {
	Ref& h = *(Ref*)c;
	if (pixel) *pixel = h.viol_pixel;
	if (buffer) *buffer = h.viol_buf;
	return h.viol_count;
}

// ---- function-level entry points for known-answer tests (no state change, no draws) ---------------
void ref_homography(const Camera* ref, const Camera* src, const float* plane, float* H) {
	ComputeHomography(*ref, *src, make_float4(plane[0], plane[1], plane[2], plane[3]), H);
}
void ref_corresponding_point(const float* H, int x, int y, float* out) {
	const float2 r = ComputeCorrespondingPoint(H, make_int2(x, y));
	out[0] = r.x; out[1] = r.y;
}
float ref_ncc_old(void* c, int x, int y, int src_idx, const float* plane) {
	Ref& h = *(Ref*)c; fill_helper(h); reset_draws(h, 0, 0, -1);
	return ComputeBilateralNCCOld(make_int2(x, y), src_idx, make_float4(plane[0], plane[1], plane[2], plane[3]), &h.helper);
}
float ref_ncc_new(void* c, int x, int y, int src_idx, const float* plane) {
	Ref& h = *(Ref*)c; fill_helper(h); reset_draws(h, 0, 0, -1);
	return ComputeBilateralNCCNew(make_int2(x, y), src_idx, make_float4(plane[0], plane[1], plane[2], plane[3]), &h.helper);
}
float ref_geom_cost(void* c, int x, int y, int src_idx, const float* plane) {
	Ref& h = *(Ref*)c; fill_helper(h); reset_draws(h, 0, 0, -1);
	return ComputeGeomConsistencyCost(make_int2(x, y), src_idx, make_float4(plane[0], plane[1], plane[2], plane[3]), &h.helper);
}
// n (pixel, plane) pairs x all source views -> out[n * (num_images-1)], through ComputeMultiViewCostVectorOld
void ref_eval_cost_vectors(void* c, const int* px, const float* planes, int n, float* out) {
	Ref& h = *(Ref*)c; fill_helper(h); reset_draws(h, 0, 0, -1);
	const int S = h.num_images - 1;
	for (int i = 0; i < n; ++i) {
		float cv[MAX_IMAGES];
		for (float& v : cv) v = 2.0f;
		ComputeMultiViewCostVectorOld(make_int2(px[2 * i], px[2 * i + 1]),
			make_float4(planes[4 * i], planes[4 * i + 1], planes[4 * i + 2], planes[4 * i + 3]), cv, &h.helper);
		for (int v = 0; v < S; ++v) out[(size_t)i * S + v] = cv[v];
	}
}
int ref_bresenham(void* c, int ax, int ay, int bx, int by) {
	Ref& h = *(Ref*)c; fill_helper(h);
	return BresenhamLine(make_int2(ax, ay), make_int2(bx, by), &h.helper) ? 1 : 0;
}
int ref_point_in_triangle(int ax, int ay, int bx, int by, int cx, int cy, int px, int py) {
	return PointinTriangle(make_short2(ax, ay), make_short2(bx, by), make_short2(cx, cy), make_int2(px, py)) ? 1 : 0;
}

}  // extern "C"
