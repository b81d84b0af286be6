// dvp_jpeg_huff.hip — the input JPEGs' Huffman scan on the device (`apd --entropy-on gpu`): the launches and the memory of the
// scheme whose per-lane arithmetic is dvp_jpeg_huff.hpp (read its head first).  A lane owns a subsequence; the Huffman tables are
// copied into LDS by every work-group (3.7 KB: the lanes of a wave walk them at unrelated places, LDS serves that, the scalar cache
// would not); the bytes are read from global memory a byte at a time — a wave's lanes diverge per symbol by design, the work is
// integer and latency-bound, and what hides the latency is the number of waves in flight.
//   dvp_jh_init      the guessed entry states
//   dvp_jh_sync      a work-group per chunk of 256 subsequences: every lane runs on until its trajectory merges, a barrier per step
//   dvp_jh_round     a work-group per chunk, one lane working: a new entry state of the chunk's first lane walked through the chunk;
//                    the host repeats the launch while a state crossed a chunk boundary (the counter kChanged), up to kRoundCap
//   dvp_jh_census    blocks that begin in each lane, and the proof that the states are exact
//   dvp_jh_count     records per block at offsets[raster + 1], DC differences in scan order; the checks that raise the flag
//   dvp_jh_scan_*    the three-launch inclusive prefix sum (tile sums, their scan by one work-group, the tiles again), for the
//                    lanes' block numbers, the offsets (32-bit) and the DC differences (into 64-bit sums)
//   dvp_jh_finish_dc the predictions from the sums, restarted per segment; the +-2^25 limit
//   dvp_jh_write     the records, in raster order
// The host reads the counters once after dvp_jh_sync, once per round, and once — with the record totals — before it reserves the
// records.  Every store of the passes lies inside its array for ANY states (place_of only makes block numbers below the quota),
// so a scan whose flag is raised has written rubbish to its own arrays and nowhere else.  Plain vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <chrono>
#include <stdlib.h>

#include "dvp_jpeg_huff_run.h"

namespace dvpjh {

constexpr int kLaneGroup = 128;   // lanes per work-group of the census, count and write passes
constexpr int kScanItems = 8, kScanTile = 256 * kScanItems;

__device__ inline void load_tables(Tables* lds, const Tables* from) {
	static_assert(sizeof(Tables) % 4 == 0, "copied by words");
	const uint32_t* g = reinterpret_cast<const uint32_t*>(from);
	uint32_t* l = reinterpret_cast<uint32_t*>(lds);
	for (unsigned k = threadIdx.x; k < sizeof(Tables) / 4; k += blockDim.x) l[k] = g[k];
	__syncthreads();
}

__global__ void __launch_bounds__(256) dvp_jh_init(const Job j) {
	const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
	if (lane < j.lanes) init_lane(j, lane);
}

__global__ void __launch_bounds__(kChunkLanes) dvp_jh_sync(const Job j) {
	__shared__ Tables T;
	load_tables(&T, j.tables);
	uint32_t at = blockIdx.x * (uint32_t)kChunkLanes + threadIdx.x;
	bool active = at < j.lanes, carried = false;
	State s = active ? unpack(j.st[at]) : State{ 0, 0 };
	uint32_t steps = 0;
	for (int t = 0; t < kChunkLanes; ++t) {
		if (active) {
			active = sync_step(j, T, &at, &s, &carried);
			++steps;
		}
		if (!__syncthreads_or(active ? 1 : 0)) break;   // (the barrier between the steps: a slot stored in one is compared in the next)
	}
	if (carried) j.counters[kChanged] = 1;
	if (steps) { atomicMax(&j.counters[kLongest], steps); atomicAdd(&j.counters[kDecodes], steps); }
}

__global__ void __launch_bounds__(64) dvp_jh_round(const Job j, int from) {
	__shared__ Tables T;
	load_tables(&T, j.tables);
	if (threadIdx.x != 0) return;
	bool carried = false;
	const uint32_t decoded = round_chunk(j, T, blockIdx.x, from, &carried);
	if (carried) j.counters[kChanged] = 1;
	if (decoded) { atomicMax(&j.counters[kLongest], decoded); atomicAdd(&j.counters[kDecodes], decoded); }
}

__global__ void __launch_bounds__(kLaneGroup) dvp_jh_census(const Job j) {
	__shared__ Tables T;
	load_tables(&T, j.tables);
	const uint32_t lane = blockIdx.x * (uint32_t)kLaneGroup + threadIdx.x;
	if (lane < j.lanes && !census_lane(j, T, lane)) j.counters[kFlag] = 1;
}

__global__ void __launch_bounds__(kLaneGroup) dvp_jh_count(const Job j) {
	__shared__ Tables T;
	load_tables(&T, j.tables);
	const uint32_t lane = blockIdx.x * (uint32_t)kLaneGroup + threadIdx.x;
	if (lane < j.lanes && !count_lane(j, T, lane)) j.counters[kFlag] = 1;
}

__global__ void __launch_bounds__(256) dvp_jh_finish_dc(const Job j, int ci, uint32_t blocks) {
	const uint32_t b = blockIdx.x * 256u + threadIdx.x;
	if (b < blocks && !finish_dc(j, ci, b)) j.counters[kFlag] = 1;
}

__global__ void __launch_bounds__(kLaneGroup) dvp_jh_write(const Job j) {
	__shared__ Tables T;
	load_tables(&T, j.tables);
	const uint32_t lane = blockIdx.x * (uint32_t)kLaneGroup + threadIdx.x;
	if (lane < j.lanes) write_lane(j, T, lane);
}

// ---- the prefix sum ---------------------------------------------------------------------------------------------------------------
// part[] holds one value per lane; on return part[t] is the inclusive sum over lanes 0 ... t
template <class O>
__device__ inline void scan_256(O* part, int t) {
	for (int off = 1; off < 256; off <<= 1) {
		const O x = t >= off ? part[t - off] : (O)0;
		__syncthreads();
		part[t] += x;
		__syncthreads();
	}
}

template <class I, class O>
__global__ void __launch_bounds__(256) dvp_jh_scan_tiles(const I* in, size_t n, O* tile_sums) {
	__shared__ O part[256];
	const int t = threadIdx.x;
	const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)t * kScanItems;
	O sum = 0;
	for (int k = 0; k < kScanItems; ++k)
		if (base + k < n) sum += (O)in[base + k];
	part[t] = sum;
	__syncthreads();
	scan_256(part, t);
	if (t == 255) tile_sums[blockIdx.x] = part[255];
}

// one work-group: the tile sums become the sums of the tiles before each
template <class O>
__global__ void __launch_bounds__(256) dvp_jh_scan_sums(O* tile_sums, unsigned tiles) {
	__shared__ O part[256];
	const int t = threadIdx.x;
	O carry = 0;
	for (unsigned base = 0; base < tiles; base += 256) {
		const O v = base + t < tiles ? tile_sums[base + t] : (O)0;
		part[t] = v;
		__syncthreads();
		scan_256(part, t);
		if (base + t < tiles) tile_sums[base + t] = carry + part[t] - v;
		carry += part[255];
		__syncthreads();
	}
}

// (in == out is fine: a lane reads its items before it writes them, and no other lane's)
template <class I, class O>
__global__ void __launch_bounds__(256) dvp_jh_scan_apply(const I* in, size_t n, const O* tile_sums, O* out) {
	__shared__ O part[256];
	const int t = threadIdx.x;
	const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)t * kScanItems;
	O v[kScanItems], sum = 0;
	for (int k = 0; k < kScanItems; ++k) {
		if (base + k < n) sum += (O)in[base + k];
		v[k] = sum;
	}
	part[t] = sum;
	__syncthreads();
	scan_256(part, t);
	const O before = tile_sums[blockIdx.x] + part[t] - sum;
	for (int k = 0; k < kScanItems; ++k)
		if (base + k < n) out[base + k] = before + v[k];
}

namespace {

template <class I, class O>
bool inclusive_scan(const I* in, size_t n, O* out, O* tile_sums, hipStream_t st) {
	if (n == 0) return true;
	const unsigned tiles = (unsigned)((n + kScanTile - 1) / kScanTile);
	hipLaunchKernelGGL((dvp_jh_scan_tiles<I, O>), dim3(tiles), dim3(256), 0, st, in, n, tile_sums);
	hipLaunchKernelGGL((dvp_jh_scan_sums<O>), dim3(1), dim3(256), 0, st, tile_sums, tiles);
	hipLaunchKernelGGL((dvp_jh_scan_apply<I, O>), dim3(tiles), dim3(256), 0, st, in, n, (const O*)tile_sums, out);
	return hipGetLastError() == hipSuccess;
}

using clock_type = std::chrono::steady_clock;

int env_int(const char* name, int otherwise) {
	const char* v = getenv(name);
	return v && *v ? atoi(v) : otherwise;
}

}   // namespace

int subseq_bytes_in_use() {
	const int v = env_int("DVP_JPEG_SUBSEQ_BYTES", kSubseqBytes);
	return v == 64 || v == 128 || v == 256 || v == 512 ? v : kSubseqBytes;
}
bool serialised_run() { return env_int("DVP_JPEG_ENTROPY_SERIAL", 0) == 1; }

int scan_on_device(const Plan& plan, int subseq_bytes, hipStream_t st, dvpmem::DevBlock& work, dvpmem::DevBlock& recs, DeviceScan* out, ScanStats* stats, const char** why) {
	auto no = [&](const char* what) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); *why = what; return 1; };
	const bool serial = serialised_run();
	clock_type::time_point mark = clock_type::now();
	auto phase = [&](int which) {   // a serialised run waits after every phase and books its time
		if (!serial) return;
		(void)hipStreamSynchronize(st);
		const clock_type::time_point now = clock_type::now();
		stats->ms[which] += std::chrono::duration<double, std::milli>(now - mark).count();
		mark = now;
	};
	const uint32_t lanes = plan.lanes, chunks = plan.chunks;
	const int comps = plan.lay.comps;
	stats->segments = (long long)plan.segs.size();
	stats->subsequences = lanes;
	stats->chunks = chunks;
	// the layout of `work`
	dvpmem::Carve c;
	const size_t o_bytes = c.take(plan.data_bytes), o_segs = c.take(plan.segs.size() * sizeof(Seg)), o_lane_seg = c.take((size_t)lanes * 4), o_tables = c.take(sizeof(Tables));
	const size_t o_st = c.take((size_t)lanes * 8), o_carry0 = c.take((size_t)chunks * 8), o_carry1 = c.take((size_t)chunks * 8);
	const size_t o_began = c.take((size_t)lanes * 4), o_first = c.take(((size_t)lanes + 1) * 4), o_counters = c.take(kCounters * 4);
	size_t o_offsets[3] = { 0, 0, 0 }, o_dc[3] = { 0, 0, 0 }, o_sum[3] = { 0, 0, 0 }, longest = lanes;
	for (int i = 0; i < comps; ++i) {
		if (plan.lay.c[i].want) o_offsets[i] = c.take((plan.blocks[i] + 1) * 4);
		o_dc[i] = c.take(plan.blocks[i] * 4);
		o_sum[i] = c.take(plan.blocks[i] * 8);
		longest = plan.blocks[i] > longest ? plan.blocks[i] : longest;
	}
	const size_t o_tiles = c.take(((longest + kScanTile - 1) / kScanTile + 1) * 8);
	if (work.reserve(c.total, st)) return no("out of device memory");
	uint8_t* base = work.as<uint8_t>();
	Job j;
	j.bytes = base + o_bytes;
	j.segs = reinterpret_cast<const Seg*>(base + o_segs);
	j.lane_seg = reinterpret_cast<const uint32_t*>(base + o_lane_seg);
	j.tables = reinterpret_cast<const Tables*>(base + o_tables);
	j.lanes = lanes; j.segments = (uint32_t)plan.segs.size(); j.chunks = chunks; j.subseq_bytes = subseq_bytes;
	j.st = reinterpret_cast<unsigned long long*>(base + o_st);
	j.carry[0] = reinterpret_cast<unsigned long long*>(base + o_carry0);
	j.carry[1] = reinterpret_cast<unsigned long long*>(base + o_carry1);
	j.began = reinterpret_cast<uint32_t*>(base + o_began);
	j.first_block = reinterpret_cast<uint32_t*>(base + o_first);
	j.counters = reinterpret_cast<uint32_t*>(base + o_counters);
	j.lay = plan.lay;
	for (int i = 0; i < 3; ++i) {
		j.offsets[i] = i < comps && plan.lay.c[i].want ? reinterpret_cast<uint32_t*>(base + o_offsets[i]) : nullptr;
		j.dc[i] = i < comps ? reinterpret_cast<int32_t*>(base + o_dc[i]) : nullptr;
		j.dc_sum[i] = i < comps ? reinterpret_cast<long long*>(base + o_sum[i]) : nullptr;
		j.records[i] = nullptr;
	}
	void* tiles = base + o_tiles;
	// upload
	bool ok = hipMemcpyAsync(base + o_bytes, plan.data, plan.data_bytes, hipMemcpyHostToDevice, st) == hipSuccess;
	ok = ok && hipMemcpyAsync(base + o_segs, plan.segs.data(), plan.segs.size() * sizeof(Seg), hipMemcpyHostToDevice, st) == hipSuccess;
	ok = ok && hipMemcpyAsync(base + o_lane_seg, plan.lane_seg.data(), (size_t)lanes * 4, hipMemcpyHostToDevice, st) == hipSuccess;
	ok = ok && hipMemcpyAsync(base + o_tables, &plan.tables, sizeof(Tables), hipMemcpyHostToDevice, st) == hipSuccess;
	ok = ok && hipMemsetAsync(base + o_counters, 0, kCounters * 4, st) == hipSuccess;
	ok = ok && hipMemsetAsync(base + o_first, 0, 4, st) == hipSuccess;
	for (int i = 0; i < comps; ++i)
		if (j.offsets[i]) ok = ok && hipMemsetAsync(j.offsets[i], 0, 4, st) == hipSuccess;
	if (!ok) return no("upload failed");
	stats->uploaded = (long long)(plan.data_bytes + plan.segs.size() * sizeof(Seg) + (size_t)lanes * 4 + sizeof(Tables));
	phase(kMsUpload);
	// synchronisation
	const unsigned lane_groups256 = (lanes + 255u) / 256u, lane_groups = (lanes + (unsigned)kLaneGroup - 1u) / (unsigned)kLaneGroup;
	uint32_t counters[kCounters];
	auto read_counters = [&]() {
		return hipMemcpyAsync(counters, base + o_counters, sizeof(counters), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
	};
	hipLaunchKernelGGL(dvp_jh_init, dim3(lane_groups256), dim3(256), 0, st, j);
	hipLaunchKernelGGL(dvp_jh_sync, dim3(chunks), dim3(kChunkLanes), 0, st, j);
	if (hipGetLastError() != hipSuccess || !read_counters()) return no("launch failed");
	int cap = env_int("DVP_TEST_JPEG_SYNC_CAP", kRoundCap);
	cap = cap < 0 ? 0 : (cap > kRoundCap ? kRoundCap : cap);
	int from = 0;
	while (counters[kChanged]) {
		if (stats->rounds >= cap) return no("the synchronisation did not settle within the round cap");
		if (hipMemsetAsync(base + o_counters + 4 * kChanged, 0, 4, st) != hipSuccess) return no("launch failed");
		hipLaunchKernelGGL(dvp_jh_round, dim3(chunks), dim3(64), 0, st, j, from);
		if (hipGetLastError() != hipSuccess || !read_counters()) return no("launch failed");
		from = 1 - from;
		++stats->rounds;
	}
	stats->longest = counters[kLongest];
	stats->decodes = counters[kDecodes];
	phase(kMsSync);
	// census, block numbers, count
	hipLaunchKernelGGL(dvp_jh_census, dim3(lane_groups), dim3(kLaneGroup), 0, st, j);
	if (!inclusive_scan<uint32_t, uint32_t>(j.began, lanes, j.first_block + 1, (uint32_t*)tiles, st)) return no("launch failed");
	hipLaunchKernelGGL(dvp_jh_count, dim3(lane_groups), dim3(kLaneGroup), 0, st, j);
	if (hipGetLastError() != hipSuccess) return no("launch failed");
	phase(kMsCount);
	for (int i = 0; i < comps; ++i) {
		if (j.offsets[i] && !inclusive_scan<uint32_t, uint32_t>(j.offsets[i] + 1, plan.blocks[i], j.offsets[i] + 1, (uint32_t*)tiles, st)) return no("launch failed");
		if (!inclusive_scan<int32_t, long long>(j.dc[i], plan.blocks[i], j.dc_sum[i], (long long*)tiles, st)) return no("launch failed");
		hipLaunchKernelGGL(dvp_jh_finish_dc, dim3((unsigned)((plan.blocks[i] + 255) / 256)), dim3(256), 0, st, j, i, (uint32_t)plan.blocks[i]);
		if (hipGetLastError() != hipSuccess) return no("launch failed");
	}
	uint32_t totals[3] = { 0, 0, 0 };
	for (int i = 0; i < comps; ++i)
		if (j.offsets[i] && hipMemcpyAsync(&totals[i], j.offsets[i] + plan.blocks[i], 4, hipMemcpyDeviceToHost, st) != hipSuccess) return no("launch failed");
	if (!read_counters()) return no("launch failed");
	phase(kMsScans);
	if (counters[kFlag]) return no("the scan is not one the device path takes (flag raised)");
	// the records
	dvpmem::Carve rc;
	size_t o_records[3] = { 0, 0, 0 };
	for (int i = 0; i < comps; ++i)
		if (j.offsets[i]) o_records[i] = rc.take((size_t)totals[i] * 4);
	if (recs.reserve(rc.total, st)) return no("out of device memory");
	for (int i = 0; i < comps; ++i)
		if (j.offsets[i]) j.records[i] = reinterpret_cast<uint32_t*>(recs.as<uint8_t>() + o_records[i]);
	hipLaunchKernelGGL(dvp_jh_write, dim3(lane_groups), dim3(kLaneGroup), 0, st, j);
	if (hipGetLastError() != hipSuccess) return no("launch failed");
	phase(kMsWrite);
	for (int i = 0; i < 3; ++i) {
		out->offsets[i] = j.offsets[i];
		out->records[i] = j.records[i];
		out->offset_words[i] = j.offsets[i] ? plan.blocks[i] + 1 : 0;
		out->record_words[i] = j.offsets[i] ? totals[i] : 0;
	}
	return 0;
}

}   // namespace dvpjh
