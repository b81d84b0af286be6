// dvp_cloudeval.hip — the device half of `apd --evaluate`: nearest-neighbour distances between two point clouds in both directions
// and the counts behind accuracy / completeness / F1.  The definition, the grid and the hash live in dvp_cloudeval.hpp.
//   dvp_ce_bin          one lane per point: claim the point's cell in the open-addressing table (read the slot, atomicCAS only on an
//                       empty one), one 32-bit atomicAdd on the cloud's count of that slot; a point with a non-finite coordinate is
//                       not binned and gets its NaN
//   dvp_ce_block_sums / _scan_sums / _starts   exclusive prefix sum over the slot counts in three launches (the scan of dvp_labels.hip)
//   dvp_ce_scatter      one lane per point: its place in the cell-sorted list from the slot's start and a cursor (the count, counted
//                       down), where it leaves x, y, z and its original index as one 16-byte record
//   dvp_ce_query_wave   a wave takes 64 consecutive queries of the cell-sorted list; for each distinct cell among them 27 lanes look
//                       up the 27 neighbour cells, and every target cell is staged through LDS in chunks of 64 records, fetched once
//                       per wave; the lanes of that cell take the minimum
//   dvp_ce_query_lane   the naive form: a lane per query in file order, cells read straight from global memory (DVP_CLOUD_QUERY=lane)
//   both reduce the K comparisons per wave with a ballot and issue one 64-bit atomicAdd per tolerance per work-group
// Both clouds are binned once into the same table; each is the other's target.  Indices: a point index is below 2^31; the two clouds
// hold at most 2^30 finite points together (make_grid refuses more), so the table has at most 2^31 slots and a slot fits the 32 bits
// of slot_of, clear of kNotBinned; sums of slot counts stay below 2^31.  Device memory: one DevBlock per call, carved; the stream of a call is a StreamScope.
// DVP_CLOUD_TIMING=1 waits after every phase and prints the phases' times to stderr (tools/evaluate_timing.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dvp_mvs.h"
#include "dvp_cloudeval.hpp"
#include "dvp_cloudeval_run.h"
#include "dvp_devmem.hpp"
#include "dvp_wave.hpp"

namespace dvpce {

struct Tolerances {
	float t2[kMaxTolerances];
	int count;
};

constexpr uint32_t kNotBinned = 0xffffffffu;
constexpr int kScanLanes = 256, kScanBlock = 4 * kScanLanes;

__global__ void __launch_bounds__(256) dvp_ce_bin(const float* __restrict__ xyz, uint32_t n, const Grid g, unsigned long long* keys, uint64_t mask, uint32_t* count,
                                                  uint32_t* __restrict__ slot_of, float* __restrict__ d2) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
	if (!finite3(x, y, z)) {
		slot_of[i] = kNotBinned;
		if (d2) d2[i] = NAN;
		return;
	}
	const unsigned long long key = cell_key(g, x, y, z);
	uint64_t s = hash_key(key) & mask;
	for (;;) {   // (the table has at least as many empty slots as keys: the walk ends)
		unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == kEmptyKey) cur = atomicCAS(&keys[s], (unsigned long long)kEmptyKey, key);
		if (cur == kEmptyKey || cur == key) break;
		s = (s + 1) & mask;
	}
	atomicAdd(&count[s], 1u);
	slot_of[i] = (uint32_t)s;
}

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
__global__ void __launch_bounds__(kScanLanes) dvp_ce_block_sums(const uint32_t* __restrict__ count, size_t cap, uint32_t* __restrict__ sums) {
	__shared__ uint32_t lds[kScanLanes];
	uint32_t c[4], total;
	const uint32_t n = counts_of_lane(count, (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * 4, cap, c);
	(void)block_exclusive(n, lds, &total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one work-group: sums[b] becomes the number of points in the blocks before b, *all their number
__global__ void __launch_bounds__(kScanLanes) dvp_ce_scan_sums(uint32_t* sums, uint32_t blocks, uint32_t* all) {
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
__global__ void __launch_bounds__(kScanLanes) dvp_ce_starts(const uint32_t* __restrict__ count, size_t cap, const uint32_t* __restrict__ sums, uint32_t* __restrict__ start) {
	__shared__ uint32_t lds[kScanLanes];
	uint32_t c[4], total;
	const size_t first = (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * 4;
	const uint32_t n = counts_of_lane(count, first, cap, c);
	uint32_t before = sums[blockIdx.x] + block_exclusive(n, lds, &total);
	for (int k = 0; k < 4; ++k)
		if (first + k < cap) { start[first + k] = before; before += c[k]; }
}

// count[s] is the cell's cursor, counted down to 0: the order inside a cell is arbitrary
__global__ void __launch_bounds__(256) dvp_ce_scatter(const float* __restrict__ xyz, uint32_t n, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ start, uint32_t* count,
                                                      float4* __restrict__ sorted) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = slot_of[i];
	if (s == kNotBinned) return;
	const uint32_t at = start[s] + atomicSub(&count[s], 1u) - 1u;   // below start[s + 1] <= the points binned
	sorted[at] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float(i));
}

// the work-group's counts: every lane brings `valid` and its clipped distance
__device__ void add_counts(bool valid, float d2, const Tolerances& tol, uint32_t (*hits)[kMaxTolerances], unsigned long long* within) {
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	for (int k = 0; k < tol.count; ++k) {
		const uint32_t c = (uint32_t)__popcll(__ballot(valid && d2 <= tol.t2[k]));
		if (lane == 0) hits[w][k] = c;
	}
	__syncthreads();
	if ((int)threadIdx.x < tol.count) {
		const uint32_t sum = hits[0][threadIdx.x] + hits[1][threadIdx.x] + hits[2][threadIdx.x] + hits[3][threadIdx.x];
		if (sum) atomicAdd(&within[threadIdx.x], (unsigned long long)sum);
	}
}

__global__ void __launch_bounds__(256) dvp_ce_query_wave(const float4* __restrict__ queries, uint32_t nq, const float4* __restrict__ targets, const uint32_t* __restrict__ start,
                                                         const unsigned long long* __restrict__ keys, uint64_t mask, const Grid g, float T2, const Tolerances tol,
                                                         float* __restrict__ d2_out, unsigned long long* within) {
	__shared__ float4 stage[4][64];
	__shared__ uint32_t hits[4][kMaxTolerances];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const bool valid = i < nq;
	const float4 p = valid ? queries[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	const uint64_t key = valid ? cell_key(g, p.x, p.y, p.z) : kEmptyKey;
	float best = INFINITY;
	bool done = !valid;
	for (;;) {
		const unsigned long long todo = __ballot(!done);
		if (!todo) break;
		const int leader = __ffsll(todo) - 1;
		const uint64_t k = ((uint64_t)(uint32_t)__shfl((int)(key >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)key, leader);
		const bool mine = !done && key == k;
		uint32_t first = 0, length = 0;   // lane n < 27: the records of neighbour cell n
		if (lane < 27) {
			const uint64_t s = find_slot(keys, mask, neighbour_key(k, (int)lane));
			if (s <= mask) { first = start[s]; length = start[s + 1] - first; }
		}
		for (int n = 0; n < 27; ++n) {
			const uint32_t s = (uint32_t)__shfl((int)first, n), c = (uint32_t)__shfl((int)length, n);
			for (uint32_t base = 0; base < c; base += 64) {
				const uint32_t m = c - base < 64u ? c - base : 64u;
				if (lane < m) stage[w][lane] = targets[(size_t)s + base + lane];
				dvp::wave_sync();
				if (mine)
					for (uint32_t j = 0; j < m; ++j) {
						const float4 t = stage[w][j];
						best = keep_min(best, sq_dist(p.x, p.y, p.z, t.x, t.y, t.z));
					}
				dvp::wave_sync();
			}
		}
		done = done || mine;
	}
	const float d2 = clipped(best, T2);
	if (valid) d2_out[__float_as_uint(p.w)] = d2;
	add_counts(valid, d2, tol, hits, within);
}

__global__ void __launch_bounds__(256) dvp_ce_query_lane(const float* __restrict__ xyz, uint32_t nq, const float4* __restrict__ targets, const uint32_t* __restrict__ start,
                                                         const unsigned long long* __restrict__ keys, uint64_t mask, const Grid g, float T2, const Tolerances tol,
                                                         float* __restrict__ d2_out, unsigned long long* within) {
	__shared__ uint32_t hits[4][kMaxTolerances];
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	bool valid = i < nq;
	float x = 0.0f, y = 0.0f, z = 0.0f;
	if (valid) { x = xyz[3 * (size_t)i]; y = xyz[3 * (size_t)i + 1]; z = xyz[3 * (size_t)i + 2]; }
	valid = valid && finite3(x, y, z);   // (dvp_ce_bin has left the NaN of the others)
	float best = INFINITY;
	if (valid) {
		const uint64_t key = cell_key(g, x, y, z);
		for (int n = 0; n < 27; ++n) {
			const uint64_t s = find_slot(keys, mask, neighbour_key(key, n));
			if (s > mask) continue;
			for (uint32_t at = start[s], end = start[s + 1]; at < end; ++at) {
				const float4 t = targets[at];
				best = keep_min(best, sq_dist(x, y, z, t.x, t.y, t.z));
			}
		}
	}
	const float d2 = clipped(best, T2);
	if (valid) d2_out[i] = d2;
	add_counts(valid, d2, tol, hits, within);
}

}   // namespace dvpce

// the bounds of a large cloud from up to eight threads, each over its share of the points (min, max and a count: the same whatever the split)
static void add_bounds(dvpce::Bounds* all, const float* xyz, long long n) {
	const int workers = (int)std::min<long long>(8, n >> 20);
	if (workers <= 1) { all->add(xyz, n); return; }
	std::vector<dvpce::Bounds> part((size_t)workers);
	std::vector<std::thread> threads;
	try {
		for (int w = 0; w < workers; ++w) {
			const long long first = n * w / workers, end = n * (w + 1) / workers;
			threads.emplace_back([&part, xyz, first, end, w]() { part[(size_t)w].add(xyz + 3 * first, end - first); });
		}
	} catch (...) {   // no more threads to be had: this one does it all
		for (std::thread& t : threads) t.join();
		all->add(xyz, n);
		return;
	}
	for (std::thread& t : threads) t.join();
	for (const dvpce::Bounds& p : part) {
		all->finite += p.finite;
		for (int a = 0; a < 3; ++a) {
			if (p.lo[a] < all->lo[a]) all->lo[a] = p.lo[a];
			if (p.hi[a] > all->hi[a]) all->hi[a] = p.hi[a];
		}
	}
}

static thread_local dvpmem::CallError t_cloud_error;
static int cloud_fail(const char* who, const std::string& what) { return t_cloud_error.fail(who, what); }

extern "C" const char* dvp_cloud_last_error(void) { return t_cloud_error.c_str(); }

// cloud 0's points are queries against cloud 1, and with `both` the other way round; d2[c] / within[c] may be NULL.  With `on_device`
// the clouds are device arrays already and on_device[c] holds cloud c's bounds: nothing is read on the host and nothing uploaded.
static int cloud_run(const char* who, int device, const float* const xyz[2], const long long num[2], const float* tolerances, int num_tol, bool both, long long* const within[2],
                     long long* used, float* const d2[2], const dvpce::Bounds* on_device = nullptr, float* dev_d2_first = nullptr) {
	using namespace dvpce;
	t_cloud_error.clear();
	for (int c = 0; c < 2; ++c) {
		if (num[c] < 0 || num[c] > kMaxPoints) return cloud_fail(who, "a cloud holds 0 ... 2^31 - 1 points, got " + std::to_string(num[c]));
		if (num[c] > 0 && !xyz[c]) return cloud_fail(who, "the point arrays are required");
	}
	if (!tolerances) return cloud_fail(who, "the tolerances are required");
	const std::string what = check_tolerances(tolerances, num_tol);
	if (!what.empty()) return cloud_fail(who, what);
	const float T = tolerances[num_tol - 1], T2 = T * T;
	Tolerances tol;
	tol.count = num_tol;
	for (int k = 0; k < kMaxTolerances; ++k) tol.t2[k] = k < num_tol ? tolerances[k] * tolerances[k] : 0.0f;
	const bool timing = getenv("DVP_CLOUD_TIMING") != nullptr;
	const char* form = getenv("DVP_CLOUD_QUERY");
	const bool lane_form = form && std::string(form) == "lane";
	if (form && !lane_form && std::string(form) != "wave") return cloud_fail(who, "DVP_CLOUD_QUERY takes wave or lane");
	auto t_last = std::chrono::steady_clock::now();
	std::string report;
	Bounds bounds;
	long long finite[2];
	for (int c = 0; c < 2; ++c) {
		const long long before = bounds.finite;
		if (!on_device) add_bounds(&bounds, xyz[c], num[c]);
		else {
			bounds.finite += on_device[c].finite;
			for (int a = 0; a < 3; ++a) {
				if (on_device[c].lo[a] < bounds.lo[a]) bounds.lo[a] = on_device[c].lo[a];
				if (on_device[c].hi[a] > bounds.hi[a]) bounds.hi[a] = on_device[c].hi[a];
			}
		}
		finite[c] = bounds.finite - before;
	}
	Grid g;
	const std::string extent = make_grid(bounds, T, &g);
	if (!extent.empty()) return cloud_fail(who, extent);
	const uint64_t cap = table_capacity((uint64_t)(finite[0] + finite[1]));
	const uint32_t blocks = (uint32_t)((cap + kScanBlock - 1) / kScanBlock);

	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return cloud_fail(who, "hipSetDevice failed"); }
	dvpmem::DevBlock pool;
	dvpmem::StreamScope st;
	if (st.open()) return cloud_fail(who, "hipStreamCreate failed");
	auto lap = [&](const char* name) {   // (DVP_CLOUD_TIMING only)
		if (!timing) return;
		(void)hipStreamSynchronize(st);
		const auto now = std::chrono::steady_clock::now();
		char text[96];
		snprintf(text, sizeof text, " %s %.3f ms,", name, std::chrono::duration_cast<std::chrono::microseconds>(now - t_last).count() / 1000.0);
		report += text;
		t_last = now;
	};
	lap("bounds (host)");
	dvpmem::Carve carve;
	size_t o_xyz[2], o_count[2], o_start[2], o_slot[2], o_sorted[2], o_d2[2], o_sums[2];
	const size_t o_keys = carve.take(cap * 8), o_within = carve.take(2 * kMaxTolerances * 8);
	for (int c = 0; c < 2; ++c) {
		o_xyz[c] = carve.take(on_device ? 0 : (size_t)num[c] * 12);
		o_count[c] = carve.take(cap * 4);
		o_start[c] = carve.take((cap + 1) * 4);
		o_slot[c] = carve.take((size_t)num[c] * 4);
		o_sorted[c] = carve.take((size_t)finite[c] * 16);
		o_d2[c] = carve.take((size_t)num[c] * 4);
		o_sums[c] = carve.take((size_t)blocks * 4);
	}
	if (pool.reserve(carve.total)) return cloud_fail(who, "out of device memory (" + std::to_string(carve.total) + " bytes)");
	uint8_t* b = pool.as<uint8_t>();
	bool ok = hipMemsetAsync(b + o_keys, 0xff, cap * 8, st) == hipSuccess && hipMemsetAsync(b + o_within, 0, 2 * kMaxTolerances * 8, st) == hipSuccess;
	for (int c = 0; c < 2 && ok; ++c) {
		ok = hipMemsetAsync(b + o_count[c], 0, cap * 4, st) == hipSuccess;
		if (ok && num[c] && !on_device) ok = hipMemcpyAsync(b + o_xyz[c], xyz[c], (size_t)num[c] * 12, hipMemcpyHostToDevice, st) == hipSuccess;
	}
	if (!ok) { (void)hipGetLastError(); return cloud_fail(who, "upload failed"); }
	lap("upload");
	unsigned long long* keys = (unsigned long long*)(b + o_keys);
	const float* const points[2] = { on_device ? xyz[0] : (const float*)(b + o_xyz[0]), on_device ? xyz[1] : (const float*)(b + o_xyz[1]) };
	auto grid_of = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };
	for (int c = 0; c < 2; ++c)
		if (num[c]) hipLaunchKernelGGL(dvp_ce_bin, grid_of(num[c]), dim3(256), 0, st, points[c], (uint32_t)num[c], g, keys, cap - 1, (uint32_t*)(b + o_count[c]),
		                               (uint32_t*)(b + o_slot[c]), (float*)(b + o_d2[c]));
	lap("bin");
	for (int c = 0; c < 2; ++c) {
		uint32_t* count = (uint32_t*)(b + o_count[c]), *start = (uint32_t*)(b + o_start[c]), *sums = (uint32_t*)(b + o_sums[c]);
		hipLaunchKernelGGL(dvp_ce_block_sums, dim3(blocks), dim3(kScanLanes), 0, st, count, (size_t)cap, sums);
		hipLaunchKernelGGL(dvp_ce_scan_sums, dim3(1), dim3(kScanLanes), 0, st, sums, blocks, start + cap);
		hipLaunchKernelGGL(dvp_ce_starts, dim3(blocks), dim3(kScanLanes), 0, st, count, (size_t)cap, sums, start);
	}
	lap("scan");
	for (int c = 0; c < 2; ++c)
		if (num[c]) hipLaunchKernelGGL(dvp_ce_scatter, grid_of(num[c]), dim3(256), 0, st, points[c], (uint32_t)num[c], (const uint32_t*)(b + o_slot[c]),
		                               (const uint32_t*)(b + o_start[c]), (uint32_t*)(b + o_count[c]), (float4*)(b + o_sorted[c]));
	lap("scatter");
	for (int c = 0; c < (both ? 2 : 1); ++c) {
		const int t = 1 - c;
		unsigned long long* counts = (unsigned long long*)(b + o_within) + c * kMaxTolerances;
		if (lane_form) {
			if (num[c]) hipLaunchKernelGGL(dvp_ce_query_lane, grid_of(num[c]), dim3(256), 0, st, points[c], (uint32_t)num[c], (const float4*)(b + o_sorted[t]),
			                               (const uint32_t*)(b + o_start[t]), keys, cap - 1, g, T2, tol, (float*)(b + o_d2[c]), counts);
		} else if (finite[c]) {
			hipLaunchKernelGGL(dvp_ce_query_wave, grid_of(finite[c]), dim3(256), 0, st, (const float4*)(b + o_sorted[c]), (uint32_t)finite[c], (const float4*)(b + o_sorted[t]),
			                   (const uint32_t*)(b + o_start[t]), keys, cap - 1, g, T2, tol, (float*)(b + o_d2[c]), counts);
		}
		lap(c == 0 ? (lane_form ? "query 0 -> 1 (lane)" : "query 0 -> 1 (wave)") : (lane_form ? "query 1 -> 0 (lane)" : "query 1 -> 0 (wave)"));
	}
	if (hipGetLastError() != hipSuccess) return cloud_fail(who, "launch failed");
	unsigned long long counts[2 * kMaxTolerances];
	ok = hipMemcpyAsync(counts, b + o_within, sizeof counts, hipMemcpyDeviceToHost, st) == hipSuccess;
	for (int c = 0; c < 2 && ok; ++c)
		if (d2[c] && num[c]) ok = hipMemcpyAsync(d2[c], b + o_d2[c], (size_t)num[c] * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
	if (ok && dev_d2_first && num[0]) ok = hipMemcpyAsync(dev_d2_first, b + o_d2[0], (size_t)num[0] * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
	if (!ok || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return cloud_fail(who, "the distances could not be made or fetched");
	}
	lap("read-back");
	for (int c = 0; c < 2; ++c) {
		if (used) used[c] = finite[c];
		for (int k = 0; k < num_tol && within[c]; ++k) within[c][k] = (long long)counts[c * kMaxTolerances + k];
	}
	if (timing) fprintf(stderr, "%s timing (%lld + %lld points, %llu slots):%s\n", who, num[0], num[1], (unsigned long long)cap, report.c_str());
	return 0;
}

int dvpce::cloud_run_on_device(const char* who, int device, const float* const dev_xyz[2], const long long num[2], const Bounds bounds[2], const float* tolerances, int num_tol,
                               long long* const within[2], long long* used, float* const d2[2], float* dev_d2_first) {
	return cloud_run(who, device, dev_xyz, num, tolerances, num_tol, true, within, used, d2, bounds, dev_d2_first);
}

extern "C" int dvp_cloud_distances(int device, const float* query_xyz, long long num_query, const float* target_xyz, long long num_target, float max_distance, float* d2_out) {
	const char* who = "dvp_cloud_distances";
	if (!d2_out && num_query > 0) { t_cloud_error.clear(); return cloud_fail(who, "d2_out is required"); }
	const float* const xyz[2] = { query_xyz, target_xyz };
	const long long num[2] = { num_query, num_target };
	long long* const within[2] = { nullptr, nullptr };
	float* const d2[2] = { d2_out, nullptr };
	return cloud_run(who, device, xyz, num, &max_distance, 1, false, within, nullptr, d2);
}

extern "C" int dvp_cloud_evaluate(int device, const float* recon_xyz, long long num_recon, const float* truth_xyz, long long num_truth, const float* tolerances, int num_tol,
                                  long long* within_recon, long long* within_truth, long long* used, float* d2_recon, float* d2_truth) {
	const char* who = "dvp_cloud_evaluate";
	if (!within_recon || !within_truth || !used) { t_cloud_error.clear(); return cloud_fail(who, "within_recon, within_truth and used are required"); }
	const float* const xyz[2] = { recon_xyz, truth_xyz };
	const long long num[2] = { num_recon, num_truth };
	long long* const within[2] = { within_recon, within_truth };
	float* const d2[2] = { d2_recon, d2_truth };
	return cloud_run(who, device, xyz, num, tolerances, num_tol, true, within, used, d2);
}
