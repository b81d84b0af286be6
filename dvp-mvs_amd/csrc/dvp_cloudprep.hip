// dvp_cloudprep.hip — the device half of the preparation in front of `apd --evaluate`'s distances: finite points, transform, crop,
// voxel down-sampling.  The definition lives in dvp_cloudprep.hpp; the grid key, the hash and the table's capacity in dvp_cloudeval.hpp.
//   dvp_cp_keep         one lane per input point: the finite test, the transform, the crop test against the polygon in LDS (the edge
//                       loop is wave-uniform); one 64-bit ballot word per wave, one count per work-group, and the three stage counts
//   dvp_cp_block_sums / _scan_sums / _starts   exclusive prefix sum over the work-groups' counts in three launches (dvp_cloudeval.hip's
//                       scan restated; a scan block covers 1 024 counts)
//   dvp_cp_compact      the kept points in input order, the transform computed again: binary64 triples and their input indices when
//                       voxels follow, else the output's binary32 triples and indices at once
//   dvp_cp_bounds       per-axis minimum and maximum of the kept points: a work-group reduces, then one 64-bit atomicMin / atomicMax
//                       per axis on an order-preserving integer image of the double
//   dvp_cp_clear        empties the voxel table: keys, and per slot one 32-byte record { Q[3], n, first }
//   dvp_cp_accumulate   one lane per kept point: claim the voxel's slot (atomicCAS on an empty slot only, as dvp_ce_bin), three 64-bit
//                       atomicAdds, one 32-bit count, one 32-bit atomicMin of the kept-order index
//   dvp_cp_first        point k emits iff k == first[slot]: ballot words and work-group counts again, then the same scan
//   dvp_cp_emit         the emitting points store their voxel's centroid as binary32 and the input index, compacted
//   dvp_cp_float_bounds minimum, maximum and finite count of a prepared cloud for the distance stage's grid (dvp_cloud_evaluate_prepared)
// dvpcp::prepare_resident (dvp_cloudprep_run.h) is the same preparation for a raw cloud that lies in device memory already and a
// prepared cloud that stays there (dvp_cloudicp.hip's stages).
// Device memory: carved DevBlocks, one per stage whose size only the stage before can tell (input; kept points and table; output); the
// first two are gone before the distances start.  The stream of a call is a StreamScope.  DVP_CLOUD_TIMING=1 waits after every phase
// and prints the phases' times to stderr (tools/evaluate_timing.py).
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/dvp_mvs.h"
#include "dvp_cloudeval_run.h"
#include "dvp_cloudprep.hpp"
#include "dvp_cloudprep_run.h"
#include "dvp_devmem.hpp"

namespace dvpcp {

constexpr int kScanLanes = 256, kScanBlock = 4 * kScanLanes;
constexpr uint32_t kNoFirst = 0xffffffffu;

struct SlotRecord {
	unsigned long long Q[3];
	uint32_t n, first;
};
static_assert(sizeof(SlotRecord) == 32, "a slot record is 32 bytes");

// the point of lane i after the finite test and the transform; false: dropped.  stage[0] = finite as read, stage[1] = after the transform
__device__ bool point_of(const float* __restrict__ xyz, uint32_t i, const PointRule& r, double p[3], bool stage[2]) {
	const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
	stage[0] = dvpce::finite3(x, y, z);
	p[0] = (double)x; p[1] = (double)y; p[2] = (double)z;
	if (r.has_transform) {
		const double in[3] = { p[0], p[1], p[2] };
		transform_point(r.m, in, p);
	}
	stage[1] = stage[0] && finite1(p[0]) && finite1(p[1]) && finite1(p[2]);
	return stage[1];
}

__global__ void __launch_bounds__(256) dvp_cp_keep(const float* __restrict__ xyz, uint32_t n, const PointRule r, const double* __restrict__ uv, unsigned long long* __restrict__ words,
                                                   uint32_t* __restrict__ block_count, unsigned long long* stage_count) {
	__shared__ double poly[2 * kMaxPolygon];
	__shared__ uint32_t part[4][3];
	for (int k = threadIdx.x; k < 2 * r.num_polygon; k += 256) poly[k] = uv[k];
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	double p[3] = { 0.0, 0.0, 0.0 };
	bool stage[2] = { false, false };
	bool keep = i < n && point_of(xyz, i, r, p, stage);
	if (r.crop_axis >= 0) {
		// every lane walks all edges: the loop and the LDS reads are the same for the whole wave
		const bool in_axis = r.axis_min <= p[r.crop_axis] && p[r.crop_axis] <= r.axis_max;
		const double pu = p[r.u], pv = p[r.v];
		int crossings = 0;
		for (int e = 0; e < r.num_polygon; ++e) {
			const int j = e + 1 == r.num_polygon ? 0 : e + 1;
			crossings += edge_crossed(poly[2 * e], poly[2 * e + 1], poly[2 * j], poly[2 * j + 1], pu, pv);
		}
		keep = keep && in_axis && (crossings & 1);
	}
	const unsigned long long word = __ballot(keep);
	const uint32_t c0 = (uint32_t)__popcll(__ballot(stage[0])), c1 = (uint32_t)__popcll(__ballot(stage[1]));
	if (lane == 0) {
		const size_t at = (size_t)blockIdx.x * 4 + w;
		if (at * 64 < n) words[at] = word;
		part[w][0] = c0; part[w][1] = c1; part[w][2] = (uint32_t)__popcll(word);
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		const uint32_t sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
		if (sum) atomicAdd(&stage_count[threadIdx.x], (unsigned long long)sum);
		if (threadIdx.x == 2) block_count[blockIdx.x] = sum;
	}
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
__global__ void __launch_bounds__(kScanLanes) dvp_cp_block_sums(const uint32_t* __restrict__ count, size_t cap, uint32_t* __restrict__ sums) {
	__shared__ uint32_t lds[kScanLanes];
	uint32_t c[4], total;
	const uint32_t n = counts_of_lane(count, (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * 4, cap, c);
	(void)block_exclusive(n, lds, &total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one work-group: sums[b] becomes the number of points in the blocks before b, *all their number
__global__ void __launch_bounds__(kScanLanes) dvp_cp_scan_sums(uint32_t* sums, uint32_t blocks, uint32_t* all) {
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
__global__ void __launch_bounds__(kScanLanes) dvp_cp_starts(const uint32_t* __restrict__ count, size_t cap, const uint32_t* __restrict__ sums, uint32_t* __restrict__ start) {
	__shared__ uint32_t lds[kScanLanes];
	uint32_t c[4], total;
	const size_t first = (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * 4;
	const uint32_t n = counts_of_lane(count, first, cap, c);
	uint32_t before = sums[blockIdx.x] + block_exclusive(n, lds, &total);
	for (int k = 0; k < 4; ++k)
		if (first + k < cap) { start[first + k] = before; before += c[k]; }
}

// the place of lane i among the flagged: the work-group's start, the waves before this one, the lanes below this one.  Only valid
// for i < n; words beyond the last point's are not read.
__device__ bool place_of(const unsigned long long* __restrict__ words, const uint32_t* __restrict__ start, uint32_t i, uint32_t* at) {
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const size_t first_word = (size_t)blockIdx.x * 4;
	uint32_t before = start[blockIdx.x];
	for (uint32_t k = 0; k < w; ++k) before += (uint32_t)__popcll(words[first_word + k]);   // (k < w: a wave at or before this lane's, so a written word)
	const unsigned long long word = words[first_word + w];
	*at = before + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
	return (word >> lane) & 1ull;
}

__global__ void __launch_bounds__(256) dvp_cp_compact(const float* __restrict__ xyz, uint32_t n, const PointRule r, const unsigned long long* __restrict__ words,
                                                      const uint32_t* __restrict__ start, double* __restrict__ kept, uint32_t* __restrict__ source, float* __restrict__ out,
                                                      long long* __restrict__ out_index) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	uint32_t at;
	if (!place_of(words, start, i, &at)) return;
	double p[3];
	bool stage[2];
	(void)point_of(xyz, i, r, p, stage);
	if (kept) {
		kept[3 * (size_t)at] = p[0]; kept[3 * (size_t)at + 1] = p[1]; kept[3 * (size_t)at + 2] = p[2];
		source[at] = i;
	} else {
		out[3 * (size_t)at] = (float)p[0]; out[3 * (size_t)at + 1] = (float)p[1]; out[3 * (size_t)at + 2] = (float)p[2];
		out_index[at] = (long long)i;
	}
}

// a < b as doubles (neither NaN)  <=>  image(a) < image(b) as unsigned integers; -0 below +0
__host__ __device__ inline unsigned long long image_of(double d) {
	unsigned long long b;
	__builtin_memcpy(&b, &d, 8);
	return (b >> 63) ? ~b : b | (1ull << 63);
}
__host__ __device__ inline double double_of(unsigned long long image) {
	const unsigned long long b = (image >> 63) ? image & ~(1ull << 63) : ~image;
	double d;
	__builtin_memcpy(&d, &b, 8);
	return d;
}

// extent[a] = the minimum's image, extent[3 + a] = the maximum's (start: all ones, zero)
__global__ void __launch_bounds__(256) dvp_cp_bounds(const double* __restrict__ kept, uint32_t n, unsigned long long* extent) {
	__shared__ unsigned long long lo[256], hi[256];
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	for (int a = 0; a < 3; ++a) {
		lo[threadIdx.x] = i < n ? image_of(kept[3 * (size_t)i + a]) : ~0ull;
		hi[threadIdx.x] = i < n ? lo[threadIdx.x] : 0ull;
		__syncthreads();
		for (int d = 128; d > 0; d >>= 1) {
			if ((int)threadIdx.x < d) {
				if (lo[threadIdx.x + d] < lo[threadIdx.x]) lo[threadIdx.x] = lo[threadIdx.x + d];
				if (hi[threadIdx.x + d] > hi[threadIdx.x]) hi[threadIdx.x] = hi[threadIdx.x + d];
			}
			__syncthreads();
		}
		if (threadIdx.x == 0) {
			atomicMin(&extent[a], lo[0]);
			atomicMax(&extent[3 + a], hi[0]);
		}
		__syncthreads();
	}
}

__global__ void __launch_bounds__(256) dvp_cp_clear(unsigned long long* __restrict__ keys, SlotRecord* __restrict__ rec, size_t cap) {
	const size_t s = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (s >= cap) return;
	keys[s] = dvpce::kEmptyKey;
	SlotRecord r;
	r.Q[0] = r.Q[1] = r.Q[2] = 0ull;
	r.n = 0u;
	r.first = kNoFirst;
	rec[s] = r;
}

__global__ void __launch_bounds__(256) dvp_cp_accumulate(const double* __restrict__ kept, uint32_t n, const Voxels vx, unsigned long long* keys, uint64_t mask, SlotRecord* rec,
                                                         uint32_t* __restrict__ slot_of) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n) return;
	double i[3];
	uint64_t q[3];
	for (int a = 0; a < 3; ++a) voxel_parts(kept[3 * (size_t)k + a], vx.o[a], vx.s, &i[a], &q[a]);
	const unsigned long long key = voxel_key(i);
	uint64_t s = dvpce::hash_key(key) & mask;
	for (;;) {   // (the table has at least as many empty slots as keys: the walk ends)
		unsigned long long cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == dvpce::kEmptyKey) cur = atomicCAS(&keys[s], (unsigned long long)dvpce::kEmptyKey, key);
		if (cur == dvpce::kEmptyKey || cur == key) break;
		s = (s + 1) & mask;
	}
	SlotRecord* r = rec + s;
	for (int a = 0; a < 3; ++a) atomicAdd(&r->Q[a], (unsigned long long)q[a]);
	atomicAdd(&r->n, 1u);
	atomicMin(&r->first, k);
	slot_of[k] = (uint32_t)s;
}

__global__ void __launch_bounds__(256) dvp_cp_first(const uint32_t* __restrict__ slot_of, uint32_t n, const SlotRecord* __restrict__ rec, unsigned long long* __restrict__ words,
                                                    uint32_t* __restrict__ block_count) {
	__shared__ uint32_t part[4];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool emits = k < n && rec[slot_of[k]].first == k;
	const unsigned long long word = __ballot(emits);
	if (lane == 0) {
		const size_t at = (size_t)blockIdx.x * 4 + w;
		if (at * 64 < n) words[at] = word;
		part[w] = (uint32_t)__popcll(word);
	}
	__syncthreads();
	if (threadIdx.x == 0) block_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(256) dvp_cp_emit(const uint32_t* __restrict__ slot_of, uint32_t n, const Voxels vx, const unsigned long long* __restrict__ keys,
                                                   const SlotRecord* __restrict__ rec, const uint32_t* __restrict__ source, const unsigned long long* __restrict__ words,
                                                   const uint32_t* __restrict__ start, float* __restrict__ out, long long* __restrict__ out_index) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n) return;
	uint32_t at;
	if (!place_of(words, start, k, &at)) return;
	const uint32_t s = slot_of[k];
	const SlotRecord r = rec[s];
	const unsigned long long key = keys[s];
	for (int a = 0; a < 3; ++a) out[3 * (size_t)at + a] = (float)centroid(vx.o[a], vx.s, voxel_index_of_key(key, a), r.Q[a], r.n);
	out_index[at] = (long long)source[k];
}

// a < b as floats (neither NaN)  <=>  image(a) < image(b)
__host__ __device__ inline uint32_t image_of(float f) {
	uint32_t b;
	__builtin_memcpy(&b, &f, 4);
	return (b >> 31) ? ~b : b | (1u << 31);
}
__host__ __device__ inline float float_of(uint32_t image) {
	const uint32_t b = (image >> 31) ? image & ~(1u << 31) : ~image;
	float f;
	__builtin_memcpy(&f, &b, 4);
	return f;
}

// extent[a] / extent[3 + a] = the images of the minimum / maximum over the points with three finite coordinates, extent[6] their number
__global__ void __launch_bounds__(256) dvp_cp_float_bounds(const float* __restrict__ xyz, uint32_t n, uint32_t* extent) {
	__shared__ uint32_t lo[3][4], hi[3][4], cnt[4];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	float p[3] = { 0.0f, 0.0f, 0.0f };
	if (i < n) { p[0] = xyz[3 * (size_t)i]; p[1] = xyz[3 * (size_t)i + 1]; p[2] = xyz[3 * (size_t)i + 2]; }
	const bool ok = i < n && dvpce::finite3(p[0], p[1], p[2]);
	for (int a = 0; a < 3; ++a) {
		uint32_t l = ok ? image_of(p[a]) : 0xffffffffu, h = ok ? image_of(p[a]) : 0u;
		for (int d = 32; d > 0; d >>= 1) {
			const uint32_t ol = (uint32_t)__shfl_xor((int)l, d), oh = (uint32_t)__shfl_xor((int)h, d);
			l = ol < l ? ol : l;
			h = oh > h ? oh : h;
		}
		if (lane == 0) { lo[a][w] = l; hi[a][w] = h; }
	}
	const uint32_t c = (uint32_t)__popcll(__ballot(ok));
	if (lane == 0) cnt[w] = c;
	__syncthreads();
	if (threadIdx.x < 3) {
		const int a = threadIdx.x;
		uint32_t l = lo[a][0], h = hi[a][0];
		for (int k = 1; k < 4; ++k) { l = lo[a][k] < l ? lo[a][k] : l; h = hi[a][k] > h ? hi[a][k] : h; }
		atomicMin(&extent[a], l);
		atomicMax(&extent[3 + a], h);
	}
	if (threadIdx.x == 3) {
		const uint32_t sum = cnt[0] + cnt[1] + cnt[2] + cnt[3];
		if (sum) atomicAdd(&extent[6], sum);
	}
}

}   // namespace dvpcp

static thread_local dvpmem::CallError t_prep_error;
static int prep_fail(const char* who, const std::string& what) { return t_prep_error.fail(who, what); }

extern "C" const char* dvp_cloud_prep_last_error(void) { return t_prep_error.c_str(); }

namespace {

using namespace dvpcp;

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
};

// "" or what is wrong with the C description; *prep = its parser-independent form
std::string prep_of(const dvp_cloud_prep* c, Prep* prep) {
	if (!c) return "the preparation is required";
	prep->has_transform = c->transform != nullptr;
	for (int k = 0; k < 16 && c->transform; ++k) prep->m[k] = c->transform[k];
	prep->crop_axis = c->crop_axis;
	prep->axis_min = c->axis_min;
	prep->axis_max = c->axis_max;
	prep->voxel = c->voxel;
	if (c->crop_axis >= 0 && c->crop_axis <= 2) {
		if (c->num_polygon < kMinPolygon) return "the crop polygon needs at least 3 vertices, got " + std::to_string(c->num_polygon);
		if (c->num_polygon > kMaxPolygon) return "the crop polygon takes at most 256 vertices, got " + std::to_string(c->num_polygon);
		if (!c->polygon_xyz) return "the crop polygon is required";
		prep->polygon.assign(c->polygon_xyz, c->polygon_xyz + 3 * (size_t)c->num_polygon);
	}
	return check_prep(*prep);
}

dim3 grid_of(long long n) { return dim3((unsigned)((n + 255) / 256)); }

// exclusive prefix of count[0 .. nb) into start, the total into *all (device); sums holds ceil(nb / 1024) words
void launch_scan(hipStream_t st, const uint32_t* count, size_t nb, uint32_t* sums, uint32_t* start, uint32_t* all) {
	const uint32_t blocks = (uint32_t)((nb + kScanBlock - 1) / kScanBlock);
	if (blocks) hipLaunchKernelGGL(dvp_cp_block_sums, dim3(blocks), dim3(kScanLanes), 0, st, count, nb, sums);
	hipLaunchKernelGGL(dvp_cp_scan_sums, dim3(1), dim3(kScanLanes), 0, st, sums, blocks, all);
	if (blocks) hipLaunchKernelGGL(dvp_cp_starts, dim3(blocks), dim3(kScanLanes), 0, st, count, nb, sums, start);
}

// One cloud prepared on the device.  `out` then holds num_out float triples at offset 0 and, 256-byte aligned behind room for `num`
// triples, their input indices as long long.  Every other block is gone on return.  "" or the error.
struct Prepared {
	dvpmem::DevBlock out;
	long long num_out = 0, counts[4] = { 0, 0, 0, 0 };
	size_t o_index = 0;
	const float* xyz() const { return out.as<float>(); }
	const long long* index() const { return (const long long*)(out.as<uint8_t>() + o_index); }
};

// `resident`: xyz is in device memory already and is read where it lies
std::string prepare_on_device(hipStream_t st, const float* xyz, long long num, const Prep& prep, Prepared* res, Laps* laps, bool resident = false) {
	std::vector<double> uv;
	const PointRule rule = point_rule(prep, &uv);
	const uint32_t n = (uint32_t)num;
	const size_t nb = (size_t)((num + 255) / 256), nwords = (size_t)((num + 63) / 64), nsums = (nb + kScanBlock - 1) / kScanBlock;
	{
		dvpmem::Carve carve;
		(void)carve.take((size_t)num * 12);
		res->o_index = carve.take((size_t)num * 8);
		if (res->out.reserve(carve.total)) return "out of device memory (" + std::to_string(carve.total) + " bytes)";
	}
	res->num_out = 0;
	if (num == 0) return "";
	// stage 1: which points are kept, and where
	dvpmem::DevBlock in;
	dvpmem::Carve carve;
	const size_t o_xyz = carve.take(resident ? 0 : (size_t)num * 12), o_uv = carve.take(2 * kMaxPolygon * 8), o_words = carve.take(nwords * 8), o_count = carve.take(nb * 4),
	             o_start = carve.take(nb * 4), o_sums = carve.take((nsums + 1) * 4), o_stage = carve.take(4 * 8);
	if (in.reserve(carve.total)) return "out of device memory (" + std::to_string(carve.total) + " bytes)";
	uint8_t* a = in.as<uint8_t>();
	bool ok = (resident || hipMemcpyAsync(a + o_xyz, xyz, (size_t)num * 12, hipMemcpyHostToDevice, st) == hipSuccess) && hipMemsetAsync(a + o_stage, 0, 4 * 8, st) == hipSuccess;
	const float* in_xyz = resident ? xyz : (const float*)(a + o_xyz);
	if (ok && !uv.empty()) ok = hipMemcpyAsync(a + o_uv, uv.data(), uv.size() * 8, hipMemcpyHostToDevice, st) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); return "upload failed"; }
	laps->lap(st, "upload");
	unsigned long long* words = (unsigned long long*)(a + o_words);
	uint32_t* count = (uint32_t*)(a + o_count), *start = (uint32_t*)(a + o_start), *sums = (uint32_t*)(a + o_sums);
	unsigned long long* stage = (unsigned long long*)(a + o_stage);
	hipLaunchKernelGGL(dvp_cp_keep, grid_of(num), dim3(256), 0, st, in_xyz, n, rule, (const double*)(a + o_uv), words, count, stage);
	laps->lap(st, "keep");
	launch_scan(st, count, nb, sums, start, (uint32_t*)(stage + 3));
	unsigned long long host_stage[4];
	if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host_stage, stage, sizeof host_stage, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return "the kept points could not be counted";
	}
	laps->lap(st, "scan");
	for (int k = 0; k < 3; ++k) res->counts[k] = (long long)host_stage[k];
	const long long nk = res->counts[2];
	float* out = res->out.as<float>();
	long long* out_index = (long long*)(res->out.as<uint8_t>() + res->o_index);
	if (prep.voxel == 0.0) {
		hipLaunchKernelGGL(dvp_cp_compact, grid_of(num), dim3(256), 0, st, in_xyz, n, rule, words, start, (double*)nullptr, (uint32_t*)nullptr, out, out_index);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return "the kept points could not be stored"; }
		laps->lap(st, "compact");
		res->num_out = res->counts[3] = nk;
		return "";
	}
	const std::string many = check_kept(nk);
	if (!many.empty()) return many;
	if (nk == 0) return "";
	// stage 2: the kept points as doubles, their extent, the voxel table
	const uint64_t cap = dvpce::table_capacity((uint64_t)nk);
	const size_t kb = (size_t)((nk + 255) / 256), kwords = (size_t)((nk + 63) / 64), ksums = (kb + kScanBlock - 1) / kScanBlock;
	dvpmem::DevBlock work;
	dvpmem::Carve wc;
	const size_t o_kept = wc.take((size_t)nk * 24), o_source = wc.take((size_t)nk * 4), o_extent = wc.take(6 * 8), o_keys = wc.take(cap * 8), o_rec = wc.take(cap * 32),
	             o_slot = wc.take((size_t)nk * 4), o_kwords = wc.take(kwords * 8), o_kcount = wc.take(kb * 4), o_kstart = wc.take(kb * 4), o_ksums = wc.take((ksums + 1) * 4),
	             o_all = wc.take(4);
	if (work.reserve(wc.total)) return "out of device memory (" + std::to_string(wc.total) + " bytes)";
	uint8_t* b = work.as<uint8_t>();
	double* kept = (double*)(b + o_kept);
	uint32_t* source = (uint32_t*)(b + o_source);
	hipLaunchKernelGGL(dvp_cp_compact, grid_of(num), dim3(256), 0, st, in_xyz, n, rule, words, start, kept, source, (float*)nullptr, (long long*)nullptr);
	laps->lap(st, "compact");
	unsigned long long* extent = (unsigned long long*)(b + o_extent);
	ok = hipMemsetAsync(extent, 0xff, 3 * 8, st) == hipSuccess && hipMemsetAsync(extent + 3, 0, 3 * 8, st) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); return "the extent could not be cleared"; }
	hipLaunchKernelGGL(dvp_cp_bounds, grid_of(nk), dim3(256), 0, st, kept, (uint32_t)nk, extent);
	unsigned long long host_extent[6];
	if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host_extent, extent, sizeof host_extent, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return "the extent could not be made";
	}
	laps->lap(st, "bounds");
	double lo[3], hi[3];
	for (int k = 0; k < 3; ++k) { lo[k] = double_of(host_extent[k]); hi[k] = double_of(host_extent[3 + k]); }
	Voxels vx;
	const std::string extent_error = make_voxels(lo, hi, prep.voxel, &vx);
	if (!extent_error.empty()) return extent_error;
	unsigned long long* keys = (unsigned long long*)(b + o_keys);
	SlotRecord* rec = (SlotRecord*)(b + o_rec);
	uint32_t* slot_of = (uint32_t*)(b + o_slot);
	hipLaunchKernelGGL(dvp_cp_clear, grid_of((long long)cap), dim3(256), 0, st, keys, rec, (size_t)cap);
	hipLaunchKernelGGL(dvp_cp_accumulate, grid_of(nk), dim3(256), 0, st, (const double*)kept, (uint32_t)nk, vx, keys, cap - 1, rec, slot_of);
	laps->lap(st, "accumulate");
	unsigned long long* kw = (unsigned long long*)(b + o_kwords);
	uint32_t* kcount = (uint32_t*)(b + o_kcount), *kstart = (uint32_t*)(b + o_kstart), *all = (uint32_t*)(b + o_all);
	hipLaunchKernelGGL(dvp_cp_first, grid_of(nk), dim3(256), 0, st, (const uint32_t*)slot_of, (uint32_t)nk, (const SlotRecord*)rec, kw, kcount);
	launch_scan(st, kcount, kb, (uint32_t*)(b + o_ksums), kstart, all);
	hipLaunchKernelGGL(dvp_cp_emit, grid_of(nk), dim3(256), 0, st, (const uint32_t*)slot_of, (uint32_t)nk, vx, (const unsigned long long*)keys, (const SlotRecord*)rec,
	                   (const uint32_t*)source, (const unsigned long long*)kw, (const uint32_t*)kstart, out, out_index);
	uint32_t voxels = 0;
	if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&voxels, all, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return "the voxels could not be made";
	}
	laps->lap(st, "emit");
	res->num_out = res->counts[3] = (long long)voxels;
	return "";
}

// the bounds and the finite count of a prepared cloud; `extent` = 28 bytes of device memory.  false: it could not be done
bool float_bounds_of(hipStream_t st, uint32_t* extent, const float* xyz, long long num, dvpce::Bounds* bounds) {
	uint32_t host_extent[7];
	bool ok = hipMemsetAsync(extent, 0xff, 3 * 4, st) == hipSuccess && hipMemsetAsync(extent + 3, 0, 4 * 4, st) == hipSuccess;
	if (ok) hipLaunchKernelGGL(dvp_cp_float_bounds, grid_of(num), dim3(256), 0, st, xyz, (uint32_t)num, extent);
	ok = ok && hipGetLastError() == hipSuccess && hipMemcpyAsync(host_extent, extent, sizeof host_extent, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); return false; }
	bounds->finite = host_extent[6];
	for (int a = 0; a < 3 && bounds->finite; ++a) { bounds->lo[a] = float_of(host_extent[a]); bounds->hi[a] = float_of(host_extent[3 + a]); }
	return true;
}

std::string check_cloud(const float* xyz, long long num) {
	if (num < 0 || num > dvpce::kMaxPoints) return "a cloud holds 0 ... 2^31 - 1 points, got " + std::to_string(num);
	if (num > 0 && !xyz) return "the point arrays are required";
	return "";
}

}   // namespace

std::string dvpcp::prep_of_abi(const dvp_cloud_prep* c, Prep* prep) { return prep_of(c, prep); }

std::string dvpcp::prepare_resident(hipStream_t st, const float* dev_xyz, long long num, const Prep& prep, ResidentCloud* res) {
	Prepared p;
	Laps laps;
	std::string what = prepare_on_device(st, dev_xyz, num, prep, &p, &laps, true);
	if (!what.empty()) return what;
	if (laps.on) fprintf(stderr, "prepare (resident) timing (%lld points, %lld out):%s\n", num, p.num_out, laps.report.c_str());
	res->num = p.num_out;
	for (int k = 0; k < 4; ++k) res->counts[k] = p.counts[k];
	res->bounds = dvpce::Bounds();
	if (p.num_out) {
		dvpmem::DevBlock extent;
		if (extent.reserve(256)) return "out of device memory";
		if (!float_bounds_of(st, extent.as<uint32_t>(), p.xyz(), p.num_out, &res->bounds)) return "the prepared cloud's bounds could not be made";
	}
	res->out = std::move(p.out);
	return "";
}

extern "C" int dvp_cloud_prepare(int device, const float* xyz, long long num, const dvp_cloud_prep* prep, float* xyz_out, long long* first_index_out, long long* counts_out) {
	const char* who = "dvp_cloud_prepare";
	t_prep_error.clear();
	std::string what = check_cloud(xyz, num);
	if (!what.empty()) return prep_fail(who, what);
	if (!counts_out || (num > 0 && !xyz_out)) return prep_fail(who, "xyz_out and counts_out are required");
	Prep p;
	what = prep_of(prep, &p);
	if (!what.empty()) return prep_fail(who, what);
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return prep_fail(who, "hipSetDevice failed"); }
	Prepared res;
	dvpmem::StreamScope st;
	if (st.open()) return prep_fail(who, "hipStreamCreate failed");
	Laps laps;
	what = prepare_on_device(st, xyz, num, p, &res, &laps);
	if (!what.empty()) return prep_fail(who, what);
	bool ok = true;
	if (res.num_out) {
		ok = hipMemcpyAsync(xyz_out, res.xyz(), (size_t)res.num_out * 12, hipMemcpyDeviceToHost, st) == hipSuccess;
		if (ok && first_index_out) ok = hipMemcpyAsync(first_index_out, res.index(), (size_t)res.num_out * 8, hipMemcpyDeviceToHost, st) == hipSuccess;
		if (!ok || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return prep_fail(who, "the prepared cloud could not be fetched"); }
	}
	laps.lap(st, "read-back");
	for (int k = 0; k < 4; ++k) counts_out[k] = res.counts[k];
	if (laps.on) fprintf(stderr, "%s timing (%lld points, %lld out):%s\n", who, num, res.num_out, laps.report.c_str());
	return 0;
}

extern "C" int dvp_cloud_evaluate_prepared(int device, const float* recon_xyz, long long num_recon, const dvp_cloud_prep* prep_recon, const float* truth_xyz, long long num_truth,
                                           const dvp_cloud_prep* prep_truth, const float* tolerances, int num_tol, long long* within_recon, long long* within_truth, long long* used,
                                           float* d2_recon, float* d2_truth, long long* counts_out) {
	const char* who = "dvp_cloud_evaluate_prepared";
	t_prep_error.clear();
	const float* const host_xyz[2] = { recon_xyz, truth_xyz };
	const long long num[2] = { num_recon, num_truth };
	const dvp_cloud_prep* const preps[2] = { prep_recon, prep_truth };
	if (!within_recon || !within_truth || !used || !counts_out) return prep_fail(who, "within_recon, within_truth, used and counts_out are required");
	if (!tolerances) return prep_fail(who, "the tolerances are required");
	std::string what = dvpce::check_tolerances(tolerances, num_tol);
	if (!what.empty()) return prep_fail(who, what);
	Prep p[2];
	for (int c = 0; c < 2; ++c) {
		what = check_cloud(host_xyz[c], num[c]);
		if (what.empty()) what = prep_of(preps[c], &p[c]);
		if (!what.empty()) return prep_fail(who, what);
	}
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return prep_fail(who, "hipSetDevice failed"); }
	Prepared res[2];
	dvpmem::DevBlock extent_block;
	dvpmem::StreamScope st;
	if (st.open()) return prep_fail(who, "hipStreamCreate failed");
	Laps laps;
	dvpce::Bounds bounds[2];
	if (extent_block.reserve(2 * 256)) return prep_fail(who, "out of device memory");
	for (int c = 0; c < 2; ++c) {
		what = prepare_on_device(st, host_xyz[c], num[c], p[c], &res[c], &laps);
		if (!what.empty()) return prep_fail(who, what);
		for (int k = 0; k < 4; ++k) counts_out[4 * c + k] = res[c].counts[k];
		if (!res[c].num_out) continue;
		// the prepared cloud's bounds for the distance stage's grid: a centroid or an image may have overflowed binary32
		if (!float_bounds_of(st, (uint32_t*)(extent_block.as<uint8_t>() + 256 * c), res[c].xyz(), res[c].num_out, &bounds[c])) return prep_fail(who, "the prepared cloud's bounds could not be made");
		laps.lap(st, "bounds of the prepared");
	}
	if (laps.on) fprintf(stderr, "%s timing (%lld + %lld points, %lld + %lld prepared):%s\n", who, num[0], num[1], res[0].num_out, res[1].num_out, laps.report.c_str());
	const float* const dev_xyz[2] = { res[0].xyz(), res[1].xyz() };
	const long long num_out[2] = { res[0].num_out, res[1].num_out };
	long long* const within[2] = { within_recon, within_truth };
	float* const d2[2] = { d2_recon, d2_truth };
	if (dvpce::cloud_run_on_device(who, device, dev_xyz, num_out, bounds, tolerances, num_tol, within, used, d2) != 0) {
		t_prep_error.text = dvp_cloud_last_error();
		return 1;
	}
	return 0;
}
