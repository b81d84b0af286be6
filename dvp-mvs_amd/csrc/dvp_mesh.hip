// dvp_mesh.hip — the device half of `dvp_mesh_*`: a TSDF volume over a hashed block grid and the surface nets of its zero level.  The
// definition, the arithmetic of a sample, of a cell and of a face live in dvp_mesh.hpp; host and device compile that very text.
//   mesh_allocate   one launch per view, a lane per pixel: the blocks of the pixel's band, step after step; a wave dedupes equal keys
//                   among its lanes (leader loop over a ballot) and the leader claims the block's slot in the open-addressing table
//                   with one 64-bit atomicCAS.  A walk that finds no slot leaves a mark: the host doubles the table and runs the
//                   launches again (a set: the same whatever the table's size or the order of the claims)
//   mesh_compact    the table's keys as a list; the HOST sorts them (ascending key is the output's order) and hands them back
//   mesh_index / mesh_forward   slot -> block number, then per block the numbers of its 8 forward neighbours (itself included)
//   mesh_integrate  one work-group of 512 lanes per block, a lane per sample, views in add_view order: a gather, no atomics, the float
//                   sum in a fixed order.  A view is skipped for the whole block — a work-group-uniform test of the block's bounding
//                   sphere against the view's frustum and depth range — only when no sample of the block can see a masked pixel of it
//                   (view_misses_block in dvp_mesh.hpp: tests/mesh_host runs that text on the host)
//   mesh_cells      per block: F of the 9 x 9 x 9 samples the block's cells touch staged in LDS, active cells counted and ranked
//                   (first pass), then vertex and colour written at the block's base + rank (second pass, after the scan)
//   mesh_faces      per block: the quads owned by its samples counted, then written (the four cells' vertex numbers come from the
//                   neighbours' cell tables in global memory)
//   mesh_scan       exclusive prefix sum over the blocks' counts in one work-group
// Device memory: DevBlock owners (dvp_devmem.hpp), so DVP_TEST_SIDE_ALLOC_FAIL reaches every request; a job has its own stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/dvp_mvs.h"
#include "dvp_devmem.hpp"
#include "dvp_mesh.hpp"

namespace dvpmesh {

constexpr int kRegion = 9 * 9 * 9;

struct DevView {
	View v;
	int cullable;   // the camera has K's last row 0 0 1, no skew and an orthonormal R: the sphere test is valid
};

__device__ inline unsigned long long shfl64(unsigned long long v, int lane) {
	return ((unsigned long long)(uint32_t)__shfl((int)(v >> 32), lane) << 32) | (uint32_t)__shfl((int)(uint32_t)v, lane);
}

// marks: [0] the table is full, [1 + view] the view lifts to an index beyond the lattice
__global__ void __launch_bounds__(256) mesh_allocate(const DevView* __restrict__ views, int view, const Params p, unsigned long long* keys, uint64_t mask, unsigned* marks,
                                                     unsigned* claimed) {
	const View& v = views[view].v;
	const size_t L = (size_t)v.cols * v.rows;
	const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
	const bool valid = at < L && masked(v, at);
	const int y = valid ? (int)(at / v.cols) : 0, x = valid ? (int)(at - (size_t)y * v.cols) : 0;
	const float z = valid ? v.depth[at] : 0.0f;
	const int lane = threadIdx.x & 63;
	for (int m = -2 * p.M; m <= 2 * p.M; ++m) {
		uint64_t own = kEmptyKey;
		if (valid && !band_key(v, p, x, y, z, m, &own)) { marks[1 + view] = 1u; own = kEmptyKey; }
		const unsigned long long key = own;
		bool done = key == kEmptyKey;
		for (;;) {
			const unsigned long long todo = __ballot(!done);
			if (!todo) break;
			const int leader = __ffsll(todo) - 1;
			const unsigned long long k = shfl64(key, leader);
			if (lane == leader) {
				uint64_t s = hash_key(k) & mask, probes = 0;
				for (; probes <= mask; ++probes) {
					unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (cur == kEmptyKey) {
						cur = atomicCAS(&keys[s], (unsigned long long)kEmptyKey, k);
						if (cur == kEmptyKey) { atomicAdd(claimed, 1u); break; }
					}
					if (cur == k) break;
					s = (s + 1) & mask;
				}
				if (probes > mask) marks[0] = 1u;
			}
			done = done || key == k;
		}
	}
}

__global__ void __launch_bounds__(256) mesh_compact(const unsigned long long* __restrict__ keys, uint64_t cap, unsigned long long* __restrict__ out, unsigned* cursor, unsigned room) {
	const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (s >= cap) return;
	const unsigned long long k = keys[s];
	if (k == kEmptyKey) return;
	const unsigned i = atomicAdd(cursor, 1u);
	if (i < room) out[i] = k;
}

// the slot of `key`, or mask + 1   (the table has empty slots: the walk ends)
__device__ inline uint64_t find_slot(const unsigned long long* __restrict__ keys, uint64_t mask, uint64_t key) {
	for (uint64_t s = hash_key(key) & mask;; s = (s + 1) & mask) {
		const unsigned long long cur = keys[s];
		if (cur == key) return s;
		if (cur == kEmptyKey) return mask + 1;
	}
}

__global__ void __launch_bounds__(256) mesh_index(const unsigned long long* __restrict__ sorted, unsigned blocks, const unsigned long long* __restrict__ keys, uint64_t mask,
                                                  int* __restrict__ block_of_slot) {
	const unsigned b = blockIdx.x * 256u + threadIdx.x;
	if (b >= blocks) return;
	const uint64_t s = find_slot(keys, mask, sorted[b]);
	if (s <= mask) block_of_slot[s] = (int)b;
}

__global__ void __launch_bounds__(256) mesh_forward(const unsigned long long* __restrict__ sorted, unsigned blocks, const unsigned long long* __restrict__ keys, uint64_t mask,
                                                    const int* __restrict__ block_of_slot, int* __restrict__ forward) {
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t)blocks * 8) return;
	const uint64_t s = find_slot(keys, mask, forward_key(sorted[i >> 3], (int)(i & 7)));
	forward[i] = s <= mask ? block_of_slot[s] : -1;
}

__global__ void __launch_bounds__(512) mesh_integrate(const DevView* __restrict__ views, int num_views, const Params p, const unsigned long long* __restrict__ sorted,
                                                      float* __restrict__ sf, int* __restrict__ w, uint32_t* __restrict__ colour) {
	const size_t b = blockIdx.x;
	const int l = threadIdx.x;
	int at[3];
	key_block(sorted[b], at);
	const float P[3] = { lattice(at[0] * 8 + (l >> 6), p.s), lattice(at[1] * 8 + ((l >> 3) & 7), p.s), lattice(at[2] * 8 + (l & 7), p.s) };
	float C[3], radius;
	block_sphere(at, p.s, C, &radius);
	Sample a = { 0.0f, 0, 0u, 0u, 0u, 0u };
	for (int n = 0; n < num_views; ++n) {
		if (view_misses_block(views[n].v, views[n].cullable != 0, C, radius, p.tau)) continue;
		integrate(views[n].v, p.tau, P, &a);
	}
	const size_t i = b * kBlockSamples + l;
	sf[i] = a.sf;
	w[i] = a.w;
	colour[4 * i] = a.b; colour[4 * i + 1] = a.g; colour[4 * i + 2] = a.r; colour[4 * i + 3] = a.n;
}

// exclusive prefix of v over the work-group's 512 lanes; *total = the sum over all of them
__device__ inline uint32_t block_exclusive(uint32_t v, uint32_t* lds, uint32_t* total) {
	const int t = threadIdx.x;
	lds[t] = v;
	__syncthreads();
	for (int d = 1; d < kBlockSamples; d <<= 1) {
		const uint32_t add = t >= d ? lds[t - d] : 0u;
		__syncthreads();
		lds[t] += add;
		__syncthreads();
	}
	const uint32_t incl = lds[t];
	*total = lds[kBlockSamples - 1];
	__syncthreads();
	return incl - v;
}

// the sample at local (lx, ly, lz), each 0 ... 15, seen from block b: its index in the volume's arrays, or -1
__device__ inline long long sample_at(const int* __restrict__ forward, size_t b, int lx, int ly, int lz) {
	const int nb = forward[b * 8 + (lx >> 3) * 4 + (ly >> 3) * 2 + (lz >> 3)];
	return nb < 0 ? -1 : (long long)nb * kBlockSamples + (lx & 7) * 64 + (ly & 7) * 8 + (lz & 7);
}

// F of the block's 9 x 9 x 9 region into LDS: entry (lx * 9 + ly) * 9 + lz, NaN where the sample is absent or not valid
__device__ inline void stage_region(float* region, const int* __restrict__ forward, size_t b, const float* __restrict__ sf, const int* __restrict__ w, int min_weight) {
	for (int e = threadIdx.x; e < kRegion; e += kBlockSamples) {
		const long long i = sample_at(forward, b, e / 81, (e / 9) % 9, e % 9);
		region[e] = i < 0 ? NAN : sample_f(sf[i], w[i], min_weight);
	}
	__syncthreads();
}

struct CellArgs {
	Params p;
	const unsigned long long* sorted;
	const int* forward;
	const float* sf;
	const int* w;
	const uint32_t* colour;
	int* cell_vertex_of;                // [blocks * 512]: first pass the rank inside the block, second pass the vertex number; -1 = not active
	unsigned* count;                    // [blocks] first pass out
	const unsigned long long* base;     // [blocks] second pass in
	float* vertices;
	uint8_t* colours;
};

template <bool EMIT>
__global__ void __launch_bounds__(512) mesh_cells(const CellArgs a) {
	__shared__ float region[kRegion];
	__shared__ uint32_t scan[kBlockSamples];
	const size_t b = blockIdx.x;
	const int l = threadIdx.x, lx = l >> 6, ly = (l >> 3) & 7, lz = l & 7;
	stage_region(region, a.forward, b, a.sf, a.w, a.p.min_weight);
	float F[8];
	for (int c = 0; c < 8; ++c) F[c] = region[((lx + (c >> 2)) * 9 + ly + ((c >> 1) & 1)) * 9 + lz + (c & 1)];
	const bool active = cell_active(F);
	if (!EMIT) {
		uint32_t total;
		const uint32_t rank = block_exclusive(active ? 1u : 0u, scan, &total);
		a.cell_vertex_of[b * kBlockSamples + l] = active ? (int)rank : -1;
		if (l == 0) a.count[b] = total;
		return;
	}
	if (!active) return;
	const unsigned long long n = a.base[b] + (unsigned)a.cell_vertex_of[b * kBlockSamples + l];   // below the total the host has checked
	a.cell_vertex_of[b * kBlockSamples + l] = (int)n;
	int at[3];
	key_block(a.sorted[b], at);
	float X[3];
	cell_vertex(F, at[0] * 8 + lx, at[1] * 8 + ly, at[2] * 8 + lz, a.p.s, X);
	uint32_t sum[4] = { 0u, 0u, 0u, 0u };
	for (int c = 0; c < 8; ++c) {
		const long long i = sample_at(a.forward, b, lx + (c >> 2), ly + ((c >> 1) & 1), lz + (c & 1));   // (active: every corner exists)
		for (int e = 0; e < 4; ++e) sum[e] += a.colour[4 * i + e];
	}
	for (int e = 0; e < 3; ++e) {
		a.vertices[3 * n + e] = X[e];
		a.colours[3 * n + e] = mean_colour(sum[e], sum[3]);
	}
}

struct FaceArgs {
	Params p;
	const int* forward;
	const float* sf;
	const int* w;
	const int* cell_vertex_of;
	unsigned* count;                    // [blocks] quads, first pass out
	const unsigned long long* base;     // [blocks] quads before the block, second pass in
	int* faces;
};

template <bool EMIT>
__global__ void __launch_bounds__(512) mesh_faces(const FaceArgs a) {
	__shared__ float region[kRegion];
	__shared__ uint32_t scan[kBlockSamples];
	const size_t b = blockIdx.x;
	const int l = threadIdx.x;
	const int o[3] = { l >> 6, (l >> 3) & 7, l & 7 };
	stage_region(region, a.forward, b, a.sf, a.w, a.p.min_weight);
	const float F1 = region[((o[0] + 1) * 9 + o[1] + 1) * 9 + o[2] + 1];
	int kind[3], quad[3][4];
	uint32_t mine = 0;
	for (int ax = 0; ax < 3; ++ax) {
		int e0[3] = { o[0] + 1, o[1] + 1, o[2] + 1 };
		e0[ax] -= 1;
		kind[ax] = edge_face(region[(e0[0] * 9 + e0[1]) * 9 + e0[2]], F1);
		for (int q = 0; q < 4 && kind[ax]; ++q) {
			int d[3];
			quad_cell(ax, q, d);
			const long long i = sample_at(a.forward, b, o[0] + d[0], o[1] + d[1], o[2] + d[2]);
			quad[ax][q] = i < 0 ? -1 : a.cell_vertex_of[i];
			if (quad[ax][q] < 0) kind[ax] = 0;
		}
		mine += kind[ax] != 0;
	}
	uint32_t total;
	const uint32_t rank = block_exclusive(mine, scan, &total);
	if (!EMIT) {
		if (l == 0) a.count[b] = total;
		return;
	}
	unsigned long long n = a.base[b] + rank;
	for (int ax = 0; ax < 3; ++ax) {
		if (!kind[ax]) continue;
		int six[6];
		quad_faces(kind[ax], quad[ax], six);
		for (int e = 0; e < 6; ++e) a.faces[6 * n + e] = six[e];
		++n;
	}
}

// one work-group: base[b] = the sum of count[0 ... b - 1], *all = the sum of all
__global__ void __launch_bounds__(512) mesh_scan(const unsigned* __restrict__ count, unsigned blocks, unsigned long long* __restrict__ base, unsigned long long* all) {
	__shared__ uint32_t lds[kBlockSamples];
	unsigned long long carry = 0;
	for (unsigned first = 0; first < blocks; first += kBlockSamples) {   // (a chunk's sum is at most 512 * 1536: 32 bits hold it)
		const unsigned b = first + threadIdx.x;
		const uint32_t v = b < blocks ? count[b] : 0u;
		uint32_t total;
		const uint32_t before = block_exclusive(v, lds, &total);
		if (b < blocks) base[b] = carry + before;
		carry += total;
	}
	if (threadIdx.x == 0) *all = carry;
}

}   // namespace dvpmesh

using namespace dvpmesh;
using dvpmem::DevBlock;

struct dvp_mesh {
	int device = 0;
	Params p{};
	long long table_slots = 0;            // dvp_mesh_set_table: the table's first size (0 = from the masked pixels)
	hipStream_t stream = nullptr;
	std::vector<DevView> views;           // device pointers
	std::vector<DevBlock> view_mem;
	long long masked_pixels = 0;
	DevBlock views_dev, table, marks, sorted, block_of_slot, forward, sf, w, colour, cell_vertex_of, count, base, totals, vertices, colours, faces;
	long long blocks = 0, num_vertices = 0, num_faces = 0, regrows = 0, bytes = 0;
	double ms[3] = { 0.0, 0.0, 0.0 };
	bool built = false;
};

static thread_local dvpmem::CallError t_mesh_error;
static int mesh_fail(const char* who, const std::string& what) { return t_mesh_error.fail(who, what); }
static int mesh_memory(const char* who, size_t bytes) { return mesh_fail(who, "out of device memory (" + std::to_string(bytes) + " bytes)"); }

extern "C" {

const char* dvp_mesh_last_error(void) { return t_mesh_error.c_str(); }

int dvp_mesh_create(int device, float voxel, float truncation, int min_weight, dvp_mesh** out) {
	const char* who = "dvp_mesh_create";
	t_mesh_error.clear();
	if (!out) return mesh_fail(who, "the job pointer is required");
	*out = nullptr;
	Params p;
	const std::string what = check_params(voxel, truncation, min_weight, &p);
	if (!what.empty()) return mesh_fail(who, what);
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "hipSetDevice failed (no GPU?)"); }
	dvp_mesh* job = new dvp_mesh;
	job->device = device;
	job->p = p;
	if (hipStreamCreateWithFlags(&job->stream, hipStreamNonBlocking) != hipSuccess) {
		(void)hipGetLastError();
		delete job;
		return mesh_fail(who, "hipStreamCreate failed");
	}
	*out = job;
	return 0;
}

int dvp_mesh_destroy(dvp_mesh* job) {
	if (!job) return 0;
	(void)hipSetDevice(job->device);
	(void)hipStreamSynchronize(job->stream);
	(void)hipStreamDestroy(job->stream);
	delete job;   // frees every block
	return 0;
}

int dvp_mesh_set_table(dvp_mesh* job, long long slots) {
	const char* who = "dvp_mesh_set_table";
	t_mesh_error.clear();
	if (!job) return mesh_fail(who, "the job is required");
	if (slots < 4 || slots > (1ll << 32) || (slots & (slots - 1))) return mesh_fail(who, "the table's first size is a power of two from 4 to 2^32, got " + std::to_string(slots));
	job->table_slots = slots;
	return 0;
}

int dvp_mesh_add_view(dvp_mesh* job, const DvpCamera* cam, int cols, int rows, const float* depth, const uint8_t* mask, const uint8_t* bgr) {
	const char* who = "dvp_mesh_add_view";
	t_mesh_error.clear();
	if (!job || !cam || !depth || !mask || !bgr) return mesh_fail(who, "the job, the camera, the depth map, the mask and the colour image are required");
	const std::string what = check_view(cols, rows);
	if (!what.empty()) return mesh_fail(who, what);
	if (hipSetDevice(job->device) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "hipSetDevice failed"); }
	const size_t L = (size_t)cols * rows;
	DevView dv{};
	dv.v.cam = *cam;
	set_centre(&dv.v);
	dv.v.cols = cols;
	dv.v.rows = rows;
	dv.v.depth = depth; dv.v.mask = mask; dv.v.bgr = bgr;   // (the host's arrays, for the two lines below)
	dv.v.depth_max = masked_depth_max(dv.v);
	long long masked_here = 0;
	for (size_t p = 0; p < L; ++p) masked_here += masked(dv.v, p);
	dv.cullable = cullable(*cam);
	dvpmem::Carve carve;
	const size_t o_depth = carve.take(L * 4), o_mask = carve.take(L), o_bgr = carve.take(L * 3);
	DevBlock mem;
	if (mem.reserve(carve.total)) return mesh_memory(who, carve.total);
	uint8_t* b = mem.as<uint8_t>();
	const bool ok = hipMemcpyAsync(b + o_depth, depth, L * 4, hipMemcpyHostToDevice, job->stream) == hipSuccess &&
	                hipMemcpyAsync(b + o_mask, mask, L, hipMemcpyHostToDevice, job->stream) == hipSuccess &&
	                hipMemcpyAsync(b + o_bgr, bgr, L * 3, hipMemcpyHostToDevice, job->stream) == hipSuccess;
	if (hipStreamSynchronize(job->stream) != hipSuccess || !ok) { (void)hipGetLastError(); return mesh_fail(who, "upload failed"); }
	dv.v.depth = (const float*)(b + o_depth);
	dv.v.mask = b + o_mask;
	dv.v.bgr = b + o_bgr;
	job->views.push_back(dv);
	job->view_mem.push_back(std::move(mem));
	job->masked_pixels += masked_here;
	job->bytes += (long long)carve.total;
	job->built = false;
	return 0;
}

int dvp_mesh_build(dvp_mesh* job) {
	const char* who = "dvp_mesh_build";
	t_mesh_error.clear();
	if (!job) return mesh_fail(who, "the job is required");
	if (hipSetDevice(job->device) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "hipSetDevice failed"); }
	hipStream_t st = job->stream;
	job->built = false;
	job->blocks = job->num_vertices = job->num_faces = job->regrows = 0;
	const int nv = (int)job->views.size();
	auto now = []() { return std::chrono::steady_clock::now(); };
	auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration_cast<std::chrono::microseconds>(now() - t).count() / 1000.0; };
	auto failed = [&](const char* what) { (void)hipGetLastError(); return mesh_fail(who, what); };
	auto t0 = now();

	// ---- allocation
	const size_t views_bytes = sizeof(DevView) * (size_t)std::max(nv, 1), marks_bytes = 4 * (size_t)(nv + 2);
	if (job->views_dev.reserve(views_bytes, st)) return mesh_memory(who, views_bytes);
	if (job->marks.reserve(marks_bytes, st)) return mesh_memory(who, marks_bytes);
	if (nv && hipMemcpyAsync(job->views_dev.as<void>(), job->views.data(), sizeof(DevView) * (size_t)nv, hipMemcpyHostToDevice, st) != hipSuccess) return failed("upload failed");
	const DevView* views = job->views_dev.as<DevView>();
	uint64_t cap = 1024;
	if (job->table_slots) cap = (uint64_t)job->table_slots;
	else while (cap < (uint64_t)job->masked_pixels / 8) cap <<= 1;
	std::vector<unsigned> marks((size_t)nv + 2);
	unsigned claimed = 0;
	for (;;) {
		if (job->table.reserve(cap * 8, st)) return mesh_memory(who, cap * 8);
		if (hipMemsetAsync(job->table.as<void>(), 0xff, cap * 8, st) != hipSuccess || hipMemsetAsync(job->marks.as<void>(), 0, marks_bytes, st) != hipSuccess) return failed("memset failed");
		unsigned* d_marks = job->marks.as<unsigned>();
		for (int n = 0; n < nv; ++n) {
			const size_t L = (size_t)job->views[n].v.cols * job->views[n].v.rows;
			hipLaunchKernelGGL(mesh_allocate, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, st, views, n, job->p, job->table.as<unsigned long long>(), cap - 1, d_marks, d_marks + nv + 1);
		}
		if (hipGetLastError() != hipSuccess) return mesh_fail(who, "launch failed");
		if (hipMemcpyAsync(marks.data(), d_marks, marks_bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return failed("the allocation could not be made or fetched");
		for (int n = 0; n < nv; ++n)
			if (marks[1 + (size_t)n]) return mesh_fail(who, index_refusal(n));
		claimed = marks[(size_t)nv + 1];
		if (!marks[0] && (uint64_t)claimed * 2 <= cap) break;
		if (cap >= (1ull << 32)) return mesh_fail(who, "more than 2^31 blocks");
		cap <<= 1;   // a full (or more than half full) table: the same launches on a larger one give the same set
		++job->regrows;
	}
	const unsigned blocks = claimed;
	const size_t nb = std::max<size_t>(blocks, 1);
	if (job->sorted.reserve(nb * 8, st)) return mesh_memory(who, nb * 8);
	if (job->totals.reserve(32, st)) return mesh_memory(who, 32);
	if (hipMemsetAsync(job->totals.as<void>(), 0, 32, st) != hipSuccess) return failed("memset failed");
	std::vector<unsigned long long> keys(blocks);
	if (blocks) {
		hipLaunchKernelGGL(mesh_compact, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st, job->table.as<unsigned long long>(), cap, job->sorted.as<unsigned long long>(),
		                   job->totals.as<unsigned>(), blocks);
		if (hipGetLastError() != hipSuccess) return mesh_fail(who, "launch failed");
		if (hipMemcpyAsync(keys.data(), job->sorted.as<void>(), (size_t)blocks * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
			return failed("the block keys could not be fetched");
		std::sort(keys.begin(), keys.end());   // the output's order; between two device halves, as the label map's Hough step
		if (hipMemcpyAsync(job->sorted.as<void>(), keys.data(), (size_t)blocks * 8, hipMemcpyHostToDevice, st) != hipSuccess) return failed("upload failed");
	}
	job->blocks = blocks;
	job->ms[0] = ms_since(t0);
	t0 = now();

	// ---- integration
	const size_t samples = nb * kBlockSamples;
	if (job->block_of_slot.reserve(cap * 4, st)) return mesh_memory(who, cap * 4);
	if (job->forward.reserve(nb * 32, st)) return mesh_memory(who, nb * 32);
	if (job->sf.reserve(samples * 4, st)) return mesh_memory(who, samples * 4);
	if (job->w.reserve(samples * 4, st)) return mesh_memory(who, samples * 4);
	if (job->colour.reserve(samples * 16, st)) return mesh_memory(who, samples * 16);
	if (blocks) {
		const unsigned long long* sorted = job->sorted.as<unsigned long long>();
		hipLaunchKernelGGL(mesh_index, dim3((blocks + 255) / 256), dim3(256), 0, st, sorted, blocks, job->table.as<unsigned long long>(), cap - 1, job->block_of_slot.as<int>());
		hipLaunchKernelGGL(mesh_forward, dim3((unsigned)(((size_t)blocks * 8 + 255) / 256)), dim3(256), 0, st, sorted, blocks, job->table.as<unsigned long long>(), cap - 1,
		                   job->block_of_slot.as<int>(), job->forward.as<int>());
		hipLaunchKernelGGL(mesh_integrate, dim3(blocks), dim3(kBlockSamples), 0, st, views, nv, job->p, sorted, job->sf.as<float>(), job->w.as<int>(), job->colour.as<uint32_t>());
		if (hipGetLastError() != hipSuccess) return mesh_fail(who, "launch failed");
		if (hipStreamSynchronize(st) != hipSuccess) return failed("the integration failed");
	}
	job->ms[1] = ms_since(t0);
	t0 = now();

	// ---- extraction
	if (job->cell_vertex_of.reserve(samples * 4, st)) return mesh_memory(who, samples * 4);
	if (job->count.reserve(nb * 4, st)) return mesh_memory(who, nb * 4);
	if (job->base.reserve(nb * 8, st)) return mesh_memory(who, nb * 8);
	unsigned long long total = 0;
	unsigned long long* d_total = job->totals.as<unsigned long long>() + 1;
	if (blocks) {
		CellArgs ca{ job->p, job->sorted.as<unsigned long long>(), job->forward.as<int>(), job->sf.as<float>(), job->w.as<int>(), job->colour.as<uint32_t>(),
		             job->cell_vertex_of.as<int>(), job->count.as<unsigned>(), job->base.as<unsigned long long>(), nullptr, nullptr };
		hipLaunchKernelGGL(mesh_cells<false>, dim3(blocks), dim3(kBlockSamples), 0, st, ca);
		hipLaunchKernelGGL(mesh_scan, dim3(1), dim3(kBlockSamples), 0, st, job->count.as<unsigned>(), blocks, job->base.as<unsigned long long>(), d_total);
		if (hipGetLastError() != hipSuccess) return mesh_fail(who, "launch failed");
		if (hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return failed("the vertex count could not be fetched");
		if (total > (unsigned long long)kMaxVertices) return mesh_fail(who, vertex_refusal((long long)total));
		const size_t room = std::max<size_t>((size_t)total, 1);
		if (job->vertices.reserve(room * 12, st)) return mesh_memory(who, room * 12);
		if (job->colours.reserve(room * 3, st)) return mesh_memory(who, room * 3);
		ca.vertices = job->vertices.as<float>();
		ca.colours = job->colours.as<uint8_t>();
		hipLaunchKernelGGL(mesh_cells<true>, dim3(blocks), dim3(kBlockSamples), 0, st, ca);
		FaceArgs fa{ job->p, job->forward.as<int>(), job->sf.as<float>(), job->w.as<int>(), job->cell_vertex_of.as<int>(), job->count.as<unsigned>(), job->base.as<unsigned long long>(), nullptr };
		hipLaunchKernelGGL(mesh_faces<false>, dim3(blocks), dim3(kBlockSamples), 0, st, fa);
		hipLaunchKernelGGL(mesh_scan, dim3(1), dim3(kBlockSamples), 0, st, job->count.as<unsigned>(), blocks, job->base.as<unsigned long long>(), d_total + 1);
		if (hipGetLastError() != hipSuccess) return mesh_fail(who, "launch failed");
		unsigned long long quads = 0;
		if (hipMemcpyAsync(&quads, d_total + 1, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return failed("the face count could not be fetched");
		const size_t face_room = std::max<size_t>((size_t)quads, 1) * 24;
		if (job->faces.reserve(face_room, st)) return mesh_memory(who, face_room);
		fa.faces = job->faces.as<int>();
		hipLaunchKernelGGL(mesh_faces<true>, dim3(blocks), dim3(kBlockSamples), 0, st, fa);
		if (hipGetLastError() != hipSuccess) return mesh_fail(who, "launch failed");
		if (hipStreamSynchronize(st) != hipSuccess) return failed("the extraction failed");
		job->num_vertices = (long long)total;
		job->num_faces = (long long)quads * 2;
	}
	job->ms[2] = ms_since(t0);
	job->built = true;
	return 0;
}

long long dvp_mesh_block_count(const dvp_mesh* job) { return job && job->built ? job->blocks : -1; }
long long dvp_mesh_vertex_count(const dvp_mesh* job) { return job && job->built ? job->num_vertices : -1; }
long long dvp_mesh_face_count(const dvp_mesh* job) { return job && job->built ? job->num_faces : -1; }

static int mesh_fetch(dvp_mesh* job, const char* who, void* dst, const DevBlock& src, size_t bytes) {
	if (!dst || !bytes) return 0;
	if (hipMemcpyAsync(dst, src.as<void>(), bytes, hipMemcpyDeviceToHost, job->stream) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "download failed"); }
	return 0;
}

int dvp_mesh_download(dvp_mesh* job, float* vertices, uint8_t* colours, int* faces) {
	const char* who = "dvp_mesh_download";
	t_mesh_error.clear();
	if (!job || !job->built) return mesh_fail(who, "a built job is required");
	if ((job->num_vertices && (!vertices || !colours)) || (job->num_faces && !faces)) return mesh_fail(who, "the vertex, colour and face arrays are required");
	if (hipSetDevice(job->device) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "hipSetDevice failed"); }
	if (mesh_fetch(job, who, vertices, job->vertices, (size_t)job->num_vertices * 12) || mesh_fetch(job, who, colours, job->colours, (size_t)job->num_vertices * 3) ||
	    mesh_fetch(job, who, faces, job->faces, (size_t)job->num_faces * 12))
		return 1;
	if (hipStreamSynchronize(job->stream) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "download failed"); }
	return 0;
}

int dvp_mesh_download_volume(dvp_mesh* job, unsigned long long* keys, float* sf, int* w, unsigned* colour_sums) {
	const char* who = "dvp_mesh_download_volume";
	t_mesh_error.clear();
	if (!job || !job->built) return mesh_fail(who, "a built job is required");
	if (hipSetDevice(job->device) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "hipSetDevice failed"); }
	const size_t samples = (size_t)job->blocks * kBlockSamples;
	if (mesh_fetch(job, who, keys, job->sorted, (size_t)job->blocks * 8) || mesh_fetch(job, who, sf, job->sf, samples * 4) || mesh_fetch(job, who, w, job->w, samples * 4) ||
	    mesh_fetch(job, who, colour_sums, job->colour, samples * 16))
		return 1;
	if (hipStreamSynchronize(job->stream) != hipSuccess) { (void)hipGetLastError(); return mesh_fail(who, "download failed"); }
	return 0;
}

int dvp_mesh_timings(const dvp_mesh* job, double* ms, long long* regrows, long long* bytes) {
	t_mesh_error.clear();
	if (!job || !job->built) return mesh_fail("dvp_mesh_timings", "a built job is required");
	for (int k = 0; k < 3 && ms; ++k) ms[k] = job->ms[k];
	if (regrows) *regrows = job->regrows;
	if (bytes) {
		const DevBlock* all[] = { &job->views_dev, &job->table, &job->marks, &job->sorted, &job->block_of_slot, &job->forward, &job->sf, &job->w, &job->colour, &job->cell_vertex_of,
		                          &job->count, &job->base, &job->totals, &job->vertices, &job->colours, &job->faces };
		*bytes = job->bytes;
		for (const DevBlock* b : all) *bytes += (long long)b->capacity();
	}
	return 0;
}

}   // extern "C"
