// dvp_cloudicp.hip — the device half of `apd --evaluate --refine-alignment`: the correspondences and the sums of one ICP step, and the
// stages around them.  The definition, the solve and the stage loop live in dvp_cloudicp.hpp; the grid key, the hash and the table's
// capacity in dvp_cloudeval.hpp; the preparation of a stage's clouds is dvp_cloudprep.hip's.
//   dvp_ci_bin_targets  once per stage, one lane per target: claim the target's cell in the open-addressing table (dvp_ce_bin's
//                       scheme), one 32-bit atomicAdd on the slot's count
//   dvp_ci_image        every step, one lane per source: the image under D rounded to binary32 and its cell key, claimed in the
//                       sources' own table; a source without a finite image or outside the searched range gets "no correspondence"
//   dvp_ci_block_sums / _scan_sums / _starts   exclusive prefix sum over the slot counts in three launches (dvp_cloudeval.hip's scan
//                       restated)
//   dvp_ci_scatter      one lane per point: its place in the cell-sorted list, where it leaves x, y, z (a source: of its image) and
//                       its original index as one 16-byte record
//   dvp_ci_nearest      dvp_ce_query_wave's scheme: a wave takes 64 consecutive records of the cell-sorted sources; for each distinct
//                       cell among them the (2R + 1)^3 neighbour cells are looked up by the lanes, and every target cell is staged
//                       through LDS in chunks of 64 records, fetched once per wave; the lanes of that cell carry (best, best_index)
//                       and replace them iff e < best || (e == best && index < best_index)
//   dvp_ci_nearest_lane the naive form: a lane per source in index order, cells read straight from global memory
//                       (DVP_CLOUD_QUERY=lane); no table of the sources
//   dvp_ci_sums         a lane per source index: the leaf, the wave's xor-butterfly with 64-bit __shfl_xor (six levels of the tree),
//                       four waves through LDS (two more), one 16-double partial per work-group; the count by ballot and one integer
//                       atomicAdd per work-group
//   dvp_ci_sums_up      the partials reduced by the same tree, 256 per work-group, as many launches as the count needs
// A level of the tree is only added while it lies inside the padded range N: -0.0 + +0.0 is +0.0, so adding padding beyond N would
// change a sum of negative zeros.  No floating-point atomics.
// Device memory: carved DevBlocks per stage (the targets' table) and per step size (the sources' table, the results, the partials),
// freed between stages; the stream of a call is a StreamScope.  DVP_CLOUD_TIMING=1 waits after every phase and prints the phases'
// times to stderr (tools/evaluate_timing.py).  DVP_CLOUD_ICP_CELLS=27|125 chooses R = 1 or 2.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/dvp_mvs.h"
#include "dvp_cloudicp.hpp"
#include "dvp_cloudprep_run.h"
#include "dvp_devmem.hpp"
#include "dvp_wave.hpp"

namespace dvpci {

using dvpce::find_slot;
using dvpce::Grid;
using dvpce::kEmptyKey;

constexpr uint32_t kNotBinned = 0xffffffffu;
constexpr int kScanLanes = 256, kScanBlock = 4 * kScanLanes;

struct Increment {   // the three upper rows of D
	double m[12];
};
struct Reference {
	double c[3];
};

// claim the slot of `key` (read the slot, atomicCAS only on an empty one)
__device__ uint64_t claim_slot(unsigned long long* keys, uint64_t mask, unsigned long long key) {
	uint64_t s = dvpce::hash_key(key) & mask;
	for (;;) {   // (the table has at least as many empty slots as keys: the walk ends)
		unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == kEmptyKey) cur = atomicCAS(&keys[s], (unsigned long long)kEmptyKey, key);
		if (cur == kEmptyKey || cur == key) break;
		s = (s + 1) & mask;
	}
	return s;
}

__global__ void __launch_bounds__(256) dvp_ci_bin_targets(const float* __restrict__ xyz, uint32_t n, const Grid g, unsigned long long* keys, uint64_t mask, uint32_t* count,
                                                          uint32_t* __restrict__ slot_of) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint64_t s = claim_slot(keys, mask, dvpce::cell_key(g, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]));
	atomicAdd(&count[s], 1u);
	slot_of[i] = (uint32_t)s;
}

__global__ void __launch_bounds__(256) dvp_ci_image(const float* __restrict__ xyz, uint32_t n, const Increment D, const Cells cells, unsigned long long* keys, uint64_t mask,
                                                    uint32_t* count, uint32_t* __restrict__ slot_of, int* __restrict__ nearest, float* __restrict__ e_out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	double p[3];
	float r[3];
	if (!image_of(D.m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], p, r) || !searched(cells, r[0], r[1], r[2])) {
		slot_of[i] = kNotBinned;
		nearest[i] = -1;
		e_out[i] = INFINITY;
		return;
	}
	const uint64_t s = claim_slot(keys, mask, dvpce::cell_key(cells.g, r[0], r[1], r[2]));
	atomicAdd(&count[s], 1u);
	slot_of[i] = (uint32_t)s;
}

// ---- the three-launch exclusive scan of dvp_cloudeval.hip, restated ---------------------------------------------------------------------
// exclusive prefix of v over the work-group's lanes; *total = the sum over all of them
__device__ uint32_t block_exclusive(uint32_t v, uint32_t* lds, uint32_t* total) {
	const int t = threadIdx.x;
	lds[t] = v;
	__syncthreads();
	for (int d = 1; d < kScanLanes; d <<= 1) {
		const uint32_t add = t >= d ? lds[t - d] : 0u;
		__syncthreads();
		lds[t] += add;
		__syncthreads();
	}
	const uint32_t incl = lds[t];
	*total = lds[kScanLanes - 1];
	__syncthreads();
	return incl - v;
}
__device__ uint32_t counts_of_lane(const uint32_t* count, size_t first, size_t cap, uint32_t c[4]) {
	uint32_t n = 0;
	for (int k = 0; k < 4; ++k) {
		c[k] = first + k < cap ? count[first + k] : 0u;
		n += c[k];
	}
	return n;
}
__global__ void __launch_bounds__(kScanLanes) dvp_ci_block_sums(const uint32_t* __restrict__ count, size_t cap, uint32_t* __restrict__ sums) {
	__shared__ uint32_t lds[kScanLanes];
	uint32_t c[4], total;
	const uint32_t n = counts_of_lane(count, (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * 4, cap, c);
	(void)block_exclusive(n, lds, &total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one work-group: sums[b] becomes the number of points in the blocks before b, *all their number
__global__ void __launch_bounds__(kScanLanes) dvp_ci_scan_sums(uint32_t* sums, uint32_t blocks, uint32_t* all) {
	__shared__ uint32_t lds[kScanLanes];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < blocks; base += kScanLanes) {
		const uint32_t b = base + threadIdx.x;
		const uint32_t v = b < blocks ? sums[b] : 0u;
		uint32_t total;
		const uint32_t before = block_exclusive(v, lds, &total);
		if (b < blocks) sums[b] = carry + before;
		carry += total;
	}
	if (threadIdx.x == 0) *all = carry;   // start[cap]
}
__global__ void __launch_bounds__(kScanLanes) dvp_ci_starts(const uint32_t* __restrict__ count, size_t cap, const uint32_t* __restrict__ sums, uint32_t* __restrict__ start) {
	__shared__ uint32_t lds[kScanLanes];
	uint32_t c[4], total;
	const size_t first = (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * 4;
	const uint32_t n = counts_of_lane(count, first, cap, c);
	uint32_t before = sums[blockIdx.x] + block_exclusive(n, lds, &total);
	for (int k = 0; k < 4; ++k)
		if (first + k < cap) { start[first + k] = before; before += c[k]; }
}

// count[s] is the cell's cursor, counted down to 0: the order inside a cell is arbitrary.  `image`: the record holds the point's
// image under D (a source), else the point itself (a target).
__global__ void __launch_bounds__(256) dvp_ci_scatter(const float* __restrict__ xyz, uint32_t n, const Increment D, int image, const uint32_t* __restrict__ slot_of,
                                                      const uint32_t* __restrict__ start, uint32_t* count, float4* __restrict__ sorted) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = slot_of[i];
	if (s == kNotBinned) return;
	float r[3] = { xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2] };
	if (image) {
		double p[3];
		(void)image_of(D.m, r[0], r[1], r[2], p, r);
	}
	const uint32_t at = start[s] + atomicSub(&count[s], 1u) - 1u;   // below start[s + 1] <= the points binned
	sorted[at] = make_float4(r[0], r[1], r[2], __uint_as_float(i));
}

// *num_queries = the sources binned (the scan's total); the grid covers all n_src sources, the work-groups beyond the binned leave at once
__global__ void __launch_bounds__(256) dvp_ci_nearest(const float4* __restrict__ queries, const uint32_t* __restrict__ num_queries, const float4* __restrict__ targets,
                                                      const uint32_t* __restrict__ start, const unsigned long long* __restrict__ keys, uint64_t mask, const Cells cells, float d2max,
                                                      int* __restrict__ nearest, float* __restrict__ e_out) {
	__shared__ float4 stage[4][64];
	const uint32_t nq = *num_queries;
	if (blockIdx.x * 256u >= nq) return;
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const bool valid = i < nq;
	const float4 p = valid ? queries[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	const uint64_t key = valid ? dvpce::cell_key(cells.g, p.x, p.y, p.z) : kEmptyKey;
	const int R = cells.R, K = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);   // 27 or 125: two neighbour cells per lane at the most
	float best = INFINITY;
	uint32_t best_j = kNoTarget;
	bool done = !valid;
	for (;;) {
		const unsigned long long todo = __ballot(!done);
		if (!todo) break;
		const int leader = __ffsll(todo) - 1;
		const uint64_t k = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)key, leader);
		const bool mine = !done && key == k;
		uint32_t first[2] = { 0, 0 }, length[2] = { 0, 0 };   // lane l: the records of neighbour cells l and l + 64
		for (int h = 0; h < 2; ++h) {
			const int n = (int)lane + 64 * h;
			if (n < K) {
				const uint64_t s = find_slot(keys, mask, neighbour_of(k, n, R));
				if (s <= mask) { first[h] = start[s]; length[h] = start[s + 1] - first[h]; }
			}
		}
		for (int n = 0; n < K; ++n) {
			const uint32_t s = (uint32_t)__shfl((int)(n < 64 ? first[0] : first[1]), n & 63), c = (uint32_t)__shfl((int)(n < 64 ? length[0] : length[1]), n & 63);
			for (uint32_t base = 0; base < c; base += 64) {
				const uint32_t m = c - base < 64u ? c - base : 64u;
				if (lane < m) stage[w][lane] = targets[(size_t)s + base + lane];
				dvp::wave_sync();
				if (mine)
					for (uint32_t j = 0; j < m; ++j) {
						const float4 t = stage[w][j];
						const float e = dvpce::sq_dist(p.x, p.y, p.z, t.x, t.y, t.z);
						const uint32_t tj = __float_as_uint(t.w);
						if (closer(e, tj, best, best_j)) { best = e; best_j = tj; }
					}
				dvp::wave_sync();
			}
		}
		done = done || mine;
	}
	if (valid) {
		const bool corresponds = best_j != kNoTarget && best <= d2max;
		const uint32_t at = __float_as_uint(p.w);
		nearest[at] = corresponds ? (int)best_j : -1;
		e_out[at] = corresponds ? best : INFINITY;
	}
}

__global__ void __launch_bounds__(256) dvp_ci_nearest_lane(const float* __restrict__ xyz, uint32_t n, const Increment D, const float4* __restrict__ targets,
                                                           const uint32_t* __restrict__ start, const unsigned long long* __restrict__ keys, uint64_t mask, const Cells cells,
                                                           float d2max, int* __restrict__ nearest, float* __restrict__ e_out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	double p[3];
	float r[3], best = INFINITY;
	uint32_t best_j = kNoTarget;
	if (image_of(D.m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], p, r) && searched(cells, r[0], r[1], r[2])) {
		const uint64_t key = dvpce::cell_key(cells.g, r[0], r[1], r[2]);
		const int R = cells.R, K = (2 * R + 1) * (2 * R + 1) * (2 * R + 1);
		for (int k = 0; k < K; ++k) {
			const uint64_t s = find_slot(keys, mask, neighbour_of(key, k, R));
			if (s > mask) continue;
			for (uint32_t at = start[s], end = start[s + 1]; at < end; ++at) {
				const float4 t = targets[at];
				const float e = dvpce::sq_dist(r[0], r[1], r[2], t.x, t.y, t.z);
				const uint32_t tj = __float_as_uint(t.w);
				if (closer(e, tj, best, best_j)) { best = e; best_j = tj; }
			}
		}
	}
	const bool corresponds = best_j != kNoTarget && best <= d2max;
	nearest[i] = corresponds ? (int)best_j : -1;
	e_out[i] = corresponds ? best : INFINITY;
}

// The tree over the work-group's 256 values of 16 doubles, as far as it lies inside `span` (a power of two: the padded length of what
// this launch reduces): the wave's butterfly, then the four waves in tree order.  Lanes 0 ... 15 store out[lane].
__device__ void block_tree(double v[16], unsigned long long span, double (*lds)[16], double* __restrict__ out) {
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	for (int o = 1; o < 64; o <<= 1) {
		if (2ull * (unsigned long long)o > span) break;   // (uniform)
		for (int k = 0; k < 16; ++k) v[k] = v[k] + __shfl_xor(v[k], o);
	}
	if (lane == 0)
		for (int k = 0; k < 16; ++k) lds[w][k] = v[k];
	__syncthreads();
	if (threadIdx.x < 16) {
		const int k = threadIdx.x;
		double s = lds[0][k];
		if (span >= 128) s = s + lds[1][k];
		if (span >= 256) s = s + (lds[2][k] + lds[3][k]);
		out[k] = s;
	}
}

__global__ void __launch_bounds__(256) dvp_ci_sums(const float* __restrict__ src, uint32_t n, unsigned long long N, const Increment D, const float* __restrict__ tgt,
                                                   const int* __restrict__ nearest, const float* __restrict__ e_in, const Reference ref, double* __restrict__ partial,
                                                   unsigned long long* count) {
	__shared__ double lds[4][16];
	__shared__ uint32_t hits[4];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	double leaf[16];
	for (int k = 0; k < 16; ++k) leaf[k] = 0.0;
	const int j = i < n ? nearest[i] : -1;
	if (j >= 0) {
		double p[3];
		float r[3];
		(void)image_of(D.m, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], p, r);
		leaf_of(p, tgt[3 * (size_t)j], tgt[3 * (size_t)j + 1], tgt[3 * (size_t)j + 2], ref.c, e_in[i], leaf);
	}
	const uint32_t c = (uint32_t)__popcll(__ballot(j >= 0));
	if (lane == 0) hits[w] = c;
	block_tree(leaf, N, lds, partial + 16 * (size_t)blockIdx.x);   // (its barrier also orders hits)
	if (threadIdx.x == 16) {
		const uint32_t sum = hits[0] + hits[1] + hits[2] + hits[3];
		if (sum) atomicAdd(count, (unsigned long long)sum);
	}
}

// in: `real` values of 16 doubles, standing for `span` (a power of two >= real; the others are +0.0); out: one per work-group
__global__ void __launch_bounds__(256) dvp_ci_sums_up(const double* __restrict__ in, uint32_t real, uint32_t span, double* __restrict__ out) {
	__shared__ double lds[4][16];
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	double v[16];
	for (int k = 0; k < 16; ++k) v[k] = i < real ? in[16 * (size_t)i + k] : 0.0;
	block_tree(v, span, lds, out + 16 * (size_t)blockIdx.x);
}

}   // namespace dvpci

static thread_local dvpmem::CallError t_icp_error;
static int icp_fail(const char* who, const std::string& what) { return t_icp_error.fail(who, what); }

extern "C" const char* dvp_cloud_icp_last_error(void) { return t_icp_error.c_str(); }

namespace {

using namespace dvpci;

// the phases' times of one call (DVP_CLOUD_TIMING only)
struct Laps {
	bool on = getenv("DVP_CLOUD_TIMING") != nullptr;
	std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
	std::string report;
	void lap(hipStream_t st, const char* name) {
		if (!on) return;
		(void)hipStreamSynchronize(st);
		const auto now = std::chrono::steady_clock::now();
		char text[96];
		snprintf(text, sizeof text, " %s %.3f ms,", name, std::chrono::duration_cast<std::chrono::microseconds>(now - last).count() / 1000.0);
		report += text;
		last = now;
	}
	void print(const char* what, long long a, long long b) {
		if (on) fprintf(stderr, "%s timing (%lld sources, %lld targets):%s\n", what, a, b, report.c_str());
		report.clear();
	}
};

dim3 grid_of(long long n) { return dim3((unsigned)((n + 255) / 256)); }

// exclusive prefix of count[0 .. cap) into start[0 .. cap], the total at start[cap]
void launch_scan(hipStream_t st, const uint32_t* count, uint64_t cap, uint32_t* sums, uint32_t* start) {
	const uint32_t blocks = (uint32_t)((cap + kScanBlock - 1) / kScanBlock);
	hipLaunchKernelGGL(dvp_ci_block_sums, dim3(blocks), dim3(kScanLanes), 0, st, count, (size_t)cap, sums);
	hipLaunchKernelGGL(dvp_ci_scan_sums, dim3(1), dim3(kScanLanes), 0, st, sums, blocks, start + cap);
	hipLaunchKernelGGL(dvp_ci_starts, dim3(blocks), dim3(kScanLanes), 0, st, count, (size_t)cap, sums, start);
}

// "" / the search form and the neighbourhood from the environment
std::string forms_from_environment(bool* lane_form, int* R) {
	const char* form = getenv("DVP_CLOUD_QUERY");
	*lane_form = form && std::string(form) == "lane";
	if (form && !*lane_form && std::string(form) != "wave") return "DVP_CLOUD_QUERY takes wave or lane";
	*R = cells_radius_from_environment();
	if (!*R) return "DVP_CLOUD_ICP_CELLS takes 27 or 125";
	return "";
}

// One stage's targets binned on the device, and the steps against them.
struct DeviceStage {
	dvpmem::DevBlock table, work;   // the targets' cells; the sources' cells, the results and the partials of a step
	const float* tgt = nullptr;
	long long nt = 0;
	Cells cells;
	Reference ref;
	float d2max = 0.0f;
	bool lane_form = false;
	uint64_t cap = 0;
	size_t o_keys = 0, o_start = 0, o_sorted = 0;
	Laps laps;

	void release() { table.release(); work.release(); }

	// tgt: nt finite points in device memory within `b`
	std::string open(hipStream_t st, const float* dev_tgt, long long num_tgt, const dvpce::Bounds& b, float d, int R, bool lane) {
		tgt = dev_tgt;
		nt = num_tgt;
		lane_form = lane;
		d2max = d * d;
		std::string what = check_targets(b, nt);
		if (what.empty()) what = make_cells(b, d, R, &cells);
		if (!what.empty()) return what;
		reference_point(b, ref.c);
		cap = dvpce::table_capacity((uint64_t)nt);
		const uint32_t blocks = (uint32_t)((cap + kScanBlock - 1) / kScanBlock);
		dvpmem::Carve carve;
		o_keys = carve.take(cap * 8);
		o_start = carve.take((cap + 1) * 4);
		o_sorted = carve.take((size_t)nt * 16);
		const size_t o_count = carve.take(cap * 4), o_slot = carve.take((size_t)nt * 4), o_sums = carve.take((size_t)blocks * 4);
		if (table.reserve(carve.total, st)) return "out of device memory (" + std::to_string(carve.total) + " bytes)";
		uint8_t* b8 = table.as<uint8_t>();
		if (hipMemsetAsync(b8 + o_keys, 0xff, cap * 8, st) != hipSuccess || hipMemsetAsync(b8 + o_count, 0, cap * 4, st) != hipSuccess) {
			(void)hipGetLastError();
			return "the targets' table could not be cleared";
		}
		unsigned long long* keys = (unsigned long long*)(b8 + o_keys);
		uint32_t* count = (uint32_t*)(b8 + o_count), *start = (uint32_t*)(b8 + o_start), *slot = (uint32_t*)(b8 + o_slot);
		if (nt) hipLaunchKernelGGL(dvp_ci_bin_targets, grid_of(nt), dim3(256), 0, st, tgt, (uint32_t)nt, cells.g, keys, cap - 1, count, slot);
		launch_scan(st, count, cap, (uint32_t*)(b8 + o_sums), start);
		const Increment none = {};
		if (nt) hipLaunchKernelGGL(dvp_ci_scatter, grid_of(nt), dim3(256), 0, st, tgt, (uint32_t)nt, none, 0, (const uint32_t*)slot, (const uint32_t*)start, count, (float4*)(b8 + o_sorted));
		if (hipGetLastError() != hipSuccess) return "launch failed";
		laps.lap(st, "targets binned");
		return "";
	}

	// src: ns points in device memory.  nearest_host / e_host (may be NULL) receive ns entries.
	std::string step(hipStream_t st, const float* src, long long ns, const double* D, double sums[16], long long* n, int* nearest_host, float* e_host) {
		for (int k = 0; k < 16; ++k) sums[k] = 0.0;
		*n = 0;
		if (ns == 0) return "";
		Increment inc;
		for (int k = 0; k < 12; ++k) inc.m[k] = D[k];
		const uint64_t scap = dvpce::table_capacity((uint64_t)ns);
		const uint32_t sblocks = (uint32_t)((scap + kScanBlock - 1) / kScanBlock);
		const unsigned long long N = (unsigned long long)padded(ns);
		const uint32_t groups = (uint32_t)((ns + 255) / 256);
		uint32_t span = (uint32_t)(N >= 256 ? N / 256 : 1);   // the partials stand for this many
		dvpmem::Carve carve;
		const size_t o_nearest = carve.take((size_t)ns * 4), o_e = carve.take((size_t)ns * 4), o_part = carve.take((size_t)groups * 128),
		             o_up = carve.take((size_t)((span + 255) / 256) * 128), o_n = carve.take(8);
		size_t o_skeys = 0, o_scount = 0, o_sstart = 0, o_sslot = 0, o_ssorted = 0, o_ssums = 0;
		if (!lane_form) {
			o_skeys = carve.take(scap * 8); o_scount = carve.take(scap * 4); o_sstart = carve.take((scap + 1) * 4); o_sslot = carve.take((size_t)ns * 4);
			o_ssorted = carve.take((size_t)ns * 16); o_ssums = carve.take((size_t)sblocks * 4);
		}
		if (work.reserve(carve.total, st)) return "out of device memory (" + std::to_string(carve.total) + " bytes)";
		uint8_t* w8 = work.as<uint8_t>(), *t8 = table.as<uint8_t>();
		int* nearest = (int*)(w8 + o_nearest);
		float* e = (float*)(w8 + o_e);
		const unsigned long long* tkeys = (const unsigned long long*)(t8 + o_keys);
		const uint32_t* tstart = (const uint32_t*)(t8 + o_start);
		const float4* tsorted = (const float4*)(t8 + o_sorted);
		bool ok = hipMemsetAsync(w8 + o_n, 0, 8, st) == hipSuccess;
		if (lane_form) {
			hipLaunchKernelGGL(dvp_ci_nearest_lane, grid_of(ns), dim3(256), 0, st, src, (uint32_t)ns, inc, tsorted, tstart, tkeys, cap - 1, cells, d2max, nearest, e);
			laps.lap(st, "nearest (lane)");
		} else {
			ok = ok && hipMemsetAsync(w8 + o_skeys, 0xff, scap * 8, st) == hipSuccess && hipMemsetAsync(w8 + o_scount, 0, scap * 4, st) == hipSuccess;
			if (!ok) { (void)hipGetLastError(); return "the sources' table could not be cleared"; }
			unsigned long long* skeys = (unsigned long long*)(w8 + o_skeys);
			uint32_t* scount = (uint32_t*)(w8 + o_scount), *sstart = (uint32_t*)(w8 + o_sstart), *sslot = (uint32_t*)(w8 + o_sslot);
			hipLaunchKernelGGL(dvp_ci_image, grid_of(ns), dim3(256), 0, st, src, (uint32_t)ns, inc, cells, skeys, scap - 1, scount, sslot, nearest, e);
			launch_scan(st, scount, scap, (uint32_t*)(w8 + o_ssums), sstart);
			hipLaunchKernelGGL(dvp_ci_scatter, grid_of(ns), dim3(256), 0, st, src, (uint32_t)ns, inc, 1, (const uint32_t*)sslot, (const uint32_t*)sstart, scount, (float4*)(w8 + o_ssorted));
			laps.lap(st, "sources ordered");
			hipLaunchKernelGGL(dvp_ci_nearest, grid_of(ns), dim3(256), 0, st, (const float4*)(w8 + o_ssorted), (const uint32_t*)(sstart + scap), tsorted, tstart, tkeys, cap - 1, cells,
			                   d2max, nearest, e);
			laps.lap(st, "nearest (wave)");
		}
		if (!ok) { (void)hipGetLastError(); return "the count could not be cleared"; }
		double* in = (double*)(w8 + o_part), *out = (double*)(w8 + o_up);
		hipLaunchKernelGGL(dvp_ci_sums, dim3(groups), dim3(256), 0, st, src, (uint32_t)ns, N, inc, tgt, (const int*)nearest, (const float*)e, ref, in, (unsigned long long*)(w8 + o_n));
		uint32_t real = groups;
		while (span > 1) {
			const uint32_t up = (span + 255) / 256;   // (a power of two, or 1)
			hipLaunchKernelGGL(dvp_ci_sums_up, dim3(up), dim3(256), 0, st, (const double*)in, real, span, out);
			real = span = up;
			double* swap = in; in = out; out = swap;   // (the first buffer holds at least as many as any later level)
		}
		if (hipGetLastError() != hipSuccess) return "launch failed";
		unsigned long long count = 0;
		ok = hipMemcpyAsync(sums, in, 128, hipMemcpyDeviceToHost, st) == hipSuccess && hipMemcpyAsync(&count, w8 + o_n, 8, hipMemcpyDeviceToHost, st) == hipSuccess;
		if (ok && nearest_host) ok = hipMemcpyAsync(nearest_host, nearest, (size_t)ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
		if (ok && e_host) ok = hipMemcpyAsync(e_host, e, (size_t)ns * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
		if (!ok || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return "the sums could not be made or fetched"; }
		laps.lap(st, "sums");
		*n = (long long)count;
		return "";
	}
};

std::string check_cloud(const float* xyz, long long num) {
	if (num < 0 || num > dvpce::kMaxPoints) return "a cloud holds 0 ... 2^31 - 1 points, got " + std::to_string(num);
	if (num > 0 && !xyz) return "the point arrays are required";
	return "";
}

// The wave form orders the sources by cell in a table of their own, whose slots are kept in 32 bits per source clear of kNotBinned
// (dvp_cloudeval.hpp's kMaxBinned): "" or why `num` sources are too many for it.
std::string check_sources(long long num, bool lane_form) {
	if (lane_form || num <= dvpce::kMaxBinned) return "";
	return "the wave form of the search orders at most " + std::to_string(dvpce::kMaxBinned) + " (2^30) sources, got " + std::to_string(num) + "; DVP_CLOUD_QUERY=lane takes them";
}

// "" or what is wrong with the C description; *prep = its parser-independent form without transform and voxel
std::string crop_of(const dvp_cloud_prep* c, dvpcp::Prep* prep) {
	if (!c) return "";
	prep->crop_axis = c->crop_axis;
	prep->axis_min = c->axis_min;
	prep->axis_max = c->axis_max;
	if (c->crop_axis >= 0 && c->crop_axis <= 2) {
		if (c->num_polygon < dvpcp::kMinPolygon) return "the crop polygon needs at least 3 vertices, got " + std::to_string(c->num_polygon);
		if (c->num_polygon > dvpcp::kMaxPolygon) return "the crop polygon takes at most 256 vertices, got " + std::to_string(c->num_polygon);
		if (!c->polygon_xyz) return "the crop polygon is required";
		prep->polygon.assign(c->polygon_xyz, c->polygon_xyz + 3 * (size_t)c->num_polygon);
	}
	return "";
}

// dvpci::refine's backend on the device: the raw clouds stay where they were uploaded, a stage's prepared clouds and tables live
// between open_stage and close_stage
struct DeviceBackend {
	hipStream_t st = nullptr;
	const float* raw[2] = { nullptr, nullptr };
	long long num[2] = { 0, 0 };
	dvpcp::Prep prep[2];
	int R = 1;
	bool lane_form = false;
	dvpcp::ResidentCloud src, tgt;
	DeviceStage stage;
	std::string open_stage(const double M[16], double voxel, float d, long long* n_src, double c[3]) {
		dvpcp::ResidentCloud* out[2] = { &src, &tgt };
		for (int k = 0; k < 2; ++k) {
			dvpcp::Prep p = prep[k];
			p.voxel = voxel;
			p.has_transform = k == 0;
			for (int e = 0; e < 16 && k == 0; ++e) p.m[e] = M[e];
			std::string what = dvpcp::check_prep(p);
			if (what.empty()) what = dvpcp::prepare_resident(st, raw[k], num[k], p, out[k]);
			if (!what.empty()) return what;
		}
		stage.laps.lap(st, "prepared");
		const std::string what = stage.open(st, tgt.xyz(), tgt.num, tgt.bounds, d, R, lane_form);
		if (!what.empty()) return what;
		for (int a = 0; a < 3; ++a) c[a] = stage.ref.c[a];
		*n_src = src.num;
		return "";
	}
	std::string step(const double D[16], double sums[16], long long* n) {
		const std::string what = stage.step(st, src.xyz(), src.num, D, sums, n, nullptr, nullptr);
		stage.laps.print("dvp_cloud_refine_alignment step", src.num, tgt.num);
		return what;
	}
	void close_stage() {
		(void)hipStreamSynchronize(st);
		stage.release();
		src.out.release();
		tgt.out.release();
	}
};

}   // namespace

extern "C" int dvp_cloud_icp_step(int device, const float* src_xyz, long long n_src, const float* tgt_xyz, long long n_tgt, const double* increment, float max_distance,
                                  int* nearest_out, float* e_out, double* sums_out, long long* count_out) {
	const char* who = "dvp_cloud_icp_step";
	t_icp_error.clear();
	std::string what = check_cloud(src_xyz, n_src);
	if (what.empty()) what = check_cloud(tgt_xyz, n_tgt);
	if (!what.empty()) return icp_fail(who, what);
	if (!sums_out || !count_out) return icp_fail(who, "sums_out and count_out are required");
	const double identity[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
	const double* D = increment ? increment : identity;
	what = check_increment(D);
	if (what.empty()) what = check_distance(max_distance);
	bool lane_form;
	int R;
	if (what.empty()) what = forms_from_environment(&lane_form, &R);
	if (what.empty()) what = check_sources(n_src, lane_form);
	if (!what.empty()) return icp_fail(who, what);
	dvpce::Bounds b;
	b.add(tgt_xyz, n_tgt);
	what = check_targets(b, n_tgt);
	if (!what.empty()) return icp_fail(who, what);
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return icp_fail(who, "hipSetDevice failed"); }
	dvpmem::DevBlock raw;
	DeviceStage stage;
	dvpmem::StreamScope st;
	if (st.open()) return icp_fail(who, "hipStreamCreate failed");
	dvpmem::Carve carve;
	const size_t o_src = carve.take((size_t)n_src * 12), o_tgt = carve.take((size_t)n_tgt * 12);
	if (raw.reserve(carve.total)) return icp_fail(who, "out of device memory (" + std::to_string(carve.total) + " bytes)");
	uint8_t* r8 = raw.as<uint8_t>();
	bool ok = true;
	if (n_src) ok = hipMemcpyAsync(r8 + o_src, src_xyz, (size_t)n_src * 12, hipMemcpyHostToDevice, st) == hipSuccess;
	if (ok && n_tgt) ok = hipMemcpyAsync(r8 + o_tgt, tgt_xyz, (size_t)n_tgt * 12, hipMemcpyHostToDevice, st) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); return icp_fail(who, "upload failed"); }
	stage.laps.lap(st, "upload");
	what = stage.open(st, (const float*)(r8 + o_tgt), n_tgt, b, max_distance, R, lane_form);
	if (what.empty()) what = stage.step(st, (const float*)(r8 + o_src), n_src, D, sums_out, count_out, nearest_out, e_out);
	if (!what.empty()) return icp_fail(who, what);
	stage.laps.print(who, n_src, n_tgt);
	return 0;
}

extern "C" int dvp_cloud_refine_alignment(int device, const float* recon_xyz, long long n_recon, const float* truth_xyz, long long n_truth, const dvp_cloud_prep* prep_recon,
                                          const dvp_cloud_prep* prep_truth, const dvp_icp_stage* stages, int num_stages, double* transform_out, dvp_icp_log* log, int log_capacity,
                                          int* log_count) {
	const char* who = "dvp_cloud_refine_alignment";
	static_assert(sizeof(dvp_icp_log) == sizeof(LogRecord) && sizeof(dvp_icp_stage) == sizeof(Stage), "the C records are the header's");
	t_icp_error.clear();
	std::string what = check_cloud(recon_xyz, n_recon);
	if (what.empty()) what = check_cloud(truth_xyz, n_truth);
	if (!what.empty()) return icp_fail(who, what);
	if (!stages || !transform_out || !log_count || (log_capacity > 0 && !log)) return icp_fail(who, "stages, transform_out, log and log_count are required");
	if (log_capacity < 0) return icp_fail(who, "log_capacity must not be negative");
	std::vector<Stage> list;
	for (int s = 0; s < num_stages && s < kMaxStages; ++s) list.push_back(Stage{ stages[s].voxel, stages[s].max_distance, stages[s].max_iterations });
	what = check_stages(list.data(), num_stages);
	if (!what.empty()) return icp_fail(who, what);
	double M[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
	if (prep_recon && prep_recon->transform)
		for (int k = 0; k < 16; ++k) M[k] = prep_recon->transform[k];
	dvpmem::DevBlock raw;
	DeviceBackend be;
	what = crop_of(prep_recon, &be.prep[0]);
	if (what.empty()) what = crop_of(prep_truth, &be.prep[1]);
	for (int k = 0; k < 2 && what.empty(); ++k) {
		dvpcp::Prep p = be.prep[k];
		for (int e = 0; e < 16 && k == 0; ++e) p.m[e] = M[e];
		p.has_transform = k == 0;
		what = dvpcp::check_prep(p);
	}
	if (what.empty()) what = forms_from_environment(&be.lane_form, &be.R);
	if (what.empty()) what = check_sources(n_recon, be.lane_form);   // (a stage's sources are no more than the raw cloud's points)
	if (!what.empty()) return icp_fail(who, what);
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return icp_fail(who, "hipSetDevice failed"); }
	dvpmem::StreamScope st;
	if (st.open()) return icp_fail(who, "hipStreamCreate failed");
	dvpmem::Carve carve;
	const size_t o_recon = carve.take((size_t)n_recon * 12), o_truth = carve.take((size_t)n_truth * 12);
	if (raw.reserve(carve.total)) return icp_fail(who, "out of device memory (" + std::to_string(carve.total) + " bytes)");
	uint8_t* r8 = raw.as<uint8_t>();
	bool ok = true;
	if (n_recon) ok = hipMemcpyAsync(r8 + o_recon, recon_xyz, (size_t)n_recon * 12, hipMemcpyHostToDevice, st) == hipSuccess;
	if (ok && n_truth) ok = hipMemcpyAsync(r8 + o_truth, truth_xyz, (size_t)n_truth * 12, hipMemcpyHostToDevice, st) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); return icp_fail(who, "upload failed"); }
	be.st = st;
	be.raw[0] = (const float*)(r8 + o_recon);
	be.raw[1] = (const float*)(r8 + o_truth);
	be.num[0] = n_recon;
	be.num[1] = n_truth;
	std::vector<LogRecord> records;
	what = refine(be, list.data(), num_stages, M, &records);   // (it has closed every stage it opened)
	if (!what.empty()) return icp_fail(who, what);
	for (int k = 0; k < 16; ++k) transform_out[k] = M[k];
	*log_count = (int)records.size();
	for (int k = 0; k < (int)records.size() && k < log_capacity; ++k) {
		log[k].stage = records[(size_t)k].stage; log[k].step = records[(size_t)k].step; log[k].n_src = records[(size_t)k].n_src; log[k].n = records[(size_t)k].n;
		log[k].rmse = records[(size_t)k].rmse;
	}
	return 0;
}
