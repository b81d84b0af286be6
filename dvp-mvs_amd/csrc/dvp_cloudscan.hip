// dvp_cloudscan.hip — the device half of `apd --evaluate --against-scans`: the range maps of the laser scans as their scanners saw
// them, the gap of every reconstructed point behind which a scanner measured a surface, and the free-space counts.  The definition
// lives in dvp_cloudscan.hpp.
//   dvp_cs_clear   the S * 6 R R map words set to +inf's bits, four words per lane
//   dvp_cs_splat   one lane per scan point: the binary64 transform and its rounding, the truth point stored into the concatenated
//                  truth array (the distance stage reads it there: the truth is uploaded once), the texel, and one 32-bit atomicMin on
//                  r2's bit pattern whose result is not used
//   dvp_cs_gaps    one lane per point: the scans' records (scanner position) staged in LDS once per work-group, a wave-uniform loop
//                  over the scans, one 4-byte gather per (point, scan), two square roots, a subtraction and a maximum
//   dvp_cs_count   free_space[k] from d2 and gap: ballot and popcount per wave, LDS per work-group, one 64-bit atomicAdd per work-group
//                  and tolerance, as dvp_cloudeval.hip counts `within`
// Indices: a texel is below 6 * 4096^2 < 2^27, a scan's map starts at s * 6 R R words (size_t); the scans hold at most 2^31 - 1 points
// together.  Device memory: DevBlocks (the maps, 24 R R bytes per scan, stay for the whole call; the raw scans go as soon as they are
// splatted); the stream of a call is a StreamScope.  The prepared clouds reach the distance stage through dvp_cloudeval_run.h, and
// d2_recon stays on the device for the count.  DVP_CLOUD_TIMING=1 waits after every phase and prints the phases' times to stderr
// (tools/evaluate_timing.py).
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/dvp_mvs.h"
#include "dvp_cloudeval_run.h"
#include "dvp_cloudprep_run.h"
#include "dvp_cloudscan.hpp"
#include "dvp_devmem.hpp"

namespace dvpcs {

struct Rows {
	double m[12];
};
struct Scanner {
	float o[3];
};
struct ScanRecord {   // 16 bytes per scan, in device memory and in LDS
	float o[3];
	uint32_t unused;
};
struct Tolerances {
	float t[dvpce::kMaxTolerances], t2[dvpce::kMaxTolerances];
	int count;
};

__global__ void __launch_bounds__(256) dvp_cs_clear(uint4* __restrict__ maps, size_t quads) {
	const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (i < quads) maps[i] = make_uint4(kInfBits, kInfBits, kInfBits, kInfBits);
}

__global__ void __launch_bounds__(256) dvp_cs_splat(const float* __restrict__ xyz, uint32_t n, const Rows rows, const Scanner sc, int R, float* __restrict__ truth,
                                                    uint32_t* map, uint32_t words) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	float g[3];
	truth_point(rows.m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], g);
	truth[3 * (size_t)i] = g[0]; truth[3 * (size_t)i + 1] = g[1]; truth[3 * (size_t)i + 2] = g[2];
	float d[3], r2;
	if (!range2(g[0], g[1], g[2], sc.o, d, &r2)) return;
	const uint32_t t = texel_of(d, R);
	if (t < words) (void)atomicMin(&map[t], __float_as_uint(r2));   // (t < words always: |su|, |sv| <= 1 and the clamp; the test costs nothing)
}

__global__ void __launch_bounds__(256) dvp_cs_gaps(const float* __restrict__ xyz, uint32_t n, const ScanRecord* __restrict__ records, int num_scans, int R,
                                                   const uint32_t* __restrict__ maps, uint32_t words, float* __restrict__ gap_out) {
	__shared__ ScanRecord rec[kMaxScans];
	if ((int)threadIdx.x < num_scans) rec[threadIdx.x] = records[threadIdx.x];
	__syncthreads();
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
	if (!dvpce::finite3(x, y, z)) { gap_out[i] = NAN; return; }
	float best = -INFINITY;
	for (int s = 0; s < num_scans; ++s) {   // the same trip count and the same LDS reads for the whole wave
		float d[3], r2;
		if (!range2(x, y, z, rec[s].o, d, &r2)) continue;
		const uint32_t t = texel_of(d, R);
		if (t >= words) continue;   // (never: see dvp_cs_splat)
		const uint32_t bits = maps[(size_t)s * words + t];
		if (bits == kInfBits) continue;
		best = keep_max(best, root(__uint_as_float(bits)) - root(r2));
	}
	gap_out[i] = best;
}

__global__ void __launch_bounds__(256) dvp_cs_count(const float* __restrict__ d2, const float* __restrict__ gap, uint32_t n, const Tolerances tol, unsigned long long* free_space) {
	__shared__ uint32_t hits[4][dvpce::kMaxTolerances];
	const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	const bool valid = i < n;
	const float d = valid ? d2[i] : 0.0f, g = valid ? gap[i] : 0.0f;
	for (int k = 0; k < tol.count; ++k) {
		const uint32_t c = (uint32_t)__popcll(__ballot(valid && !(d <= tol.t2[k]) && g > tol.t[k]));
		if (lane == 0) hits[w][k] = c;
	}
	__syncthreads();
	if ((int)threadIdx.x < tol.count) {
		const uint32_t sum = hits[0][threadIdx.x] + hits[1][threadIdx.x] + hits[2][threadIdx.x] + hits[3][threadIdx.x];
		if (sum) atomicAdd(&free_space[threadIdx.x], (unsigned long long)sum);
	}
}

}   // namespace dvpcs

static thread_local dvpmem::CallError t_scan_error;
static int scan_fail(const char* who, const std::string& what) { return t_scan_error.fail(who, what); }

extern "C" const char* dvp_cloud_scan_last_error(void) { return t_scan_error.c_str(); }

namespace {

using namespace dvpcs;

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

dim3 grid_of(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

std::string out_of_memory(size_t bytes) { return "out of device memory (" + std::to_string(bytes) + " bytes)"; }

// "" or what is wrong; *scans = the parser-independent form of the C array
std::string scans_of(const dvp_cloud_scan* c, int num_scans, int cube_size, std::vector<Scan>* scans, long long* total) {
	std::string what = check_cube(cube_size);
	if (!what.empty()) return what;
	if (num_scans < 1 || num_scans > kMaxScans) return "num_scans must be 1 ... 64, got " + std::to_string(num_scans);
	if (!c) return "the scans are required";
	scans->resize((size_t)num_scans);
	for (int s = 0; s < num_scans; ++s) {
		(*scans)[(size_t)s].xyz = c[s].xyz;
		(*scans)[(size_t)s].num = c[s].num;
		for (int k = 0; k < 16; ++k) (*scans)[(size_t)s].m[k] = c[s].transform[k];
	}
	return check_scans(scans->data(), num_scans, total);
}

// The scans on the device: `truth` then holds the truth cloud (total float triples), `maps` the S * 6 R R words and, 256-byte
// aligned behind them, the scans' records.  The raw points are gone on return.  "" or the error.
struct ScansOnDevice {
	dvpmem::DevBlock truth, maps;
	size_t o_records = 0;
	uint32_t words = 0;
	ScanRecord host_records[kMaxScans] = {};   // (uploaded from here: it outlives the stream's work)
	const uint32_t* map_bits() const { return maps.as<uint32_t>(); }
	const ScanRecord* records() const { return (const ScanRecord*)(maps.as<uint8_t>() + o_records); }
};

std::string splat_scans(hipStream_t st, const std::vector<Scan>& scans, long long total, int R, ScansOnDevice* dev, Laps* laps) {
	const int S = (int)scans.size();
	dev->words = (uint32_t)map_words(R);
	const size_t all_words = (size_t)S * dev->words;
	{
		dvpmem::Carve carve;
		(void)carve.take(all_words * 4);
		dev->o_records = carve.take(kMaxScans * sizeof(ScanRecord));
		if (dev->maps.reserve(carve.total)) return out_of_memory(carve.total);
		if (dev->truth.reserve((size_t)total * 12)) return out_of_memory((size_t)total * 12);
	}
	dvpmem::DevBlock raw;
	if (raw.reserve((size_t)total * 12)) return out_of_memory((size_t)total * 12);
	ScanRecord* records = dev->host_records;
	bool ok = true;
	size_t at = 0;
	for (int s = 0; s < S && ok; ++s) {
		scans[(size_t)s].scanner(records[s].o);
		if (scans[(size_t)s].num) ok = hipMemcpyAsync(raw.as<float>() + 3 * at, scans[(size_t)s].xyz, (size_t)scans[(size_t)s].num * 12, hipMemcpyHostToDevice, st) == hipSuccess;
		at += (size_t)scans[(size_t)s].num;
	}
	ok = ok && hipMemcpyAsync(dev->maps.as<uint8_t>() + dev->o_records, records, sizeof dev->host_records, hipMemcpyHostToDevice, st) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); return "upload failed"; }
	laps->lap(st, "upload of the scans");
	hipLaunchKernelGGL(dvp_cs_clear, grid_of(all_words / 4), dim3(256), 0, st, dev->maps.as<uint4>(), all_words / 4);
	laps->lap(st, "clear");
	at = 0;
	for (int s = 0; s < S; ++s) {
		const long long n = scans[(size_t)s].num;
		if (!n) continue;
		Rows rows;
		Scanner sc;
		for (int k = 0; k < 12; ++k) rows.m[k] = scans[(size_t)s].m[k];
		for (int k = 0; k < 3; ++k) sc.o[k] = records[s].o[k];
		hipLaunchKernelGGL(dvp_cs_splat, grid_of((size_t)n), dim3(256), 0, st, (const float*)(raw.as<float>() + 3 * at), (uint32_t)n, rows, sc, R, dev->truth.as<float>() + 3 * at,
		                   dev->maps.as<uint32_t>() + (size_t)s * dev->words, dev->words);
		at += (size_t)n;
	}
	if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return "the range maps could not be made"; }
	laps->lap(st, "splat");
	return "";
}

void launch_gaps(hipStream_t st, const float* xyz, long long n, const ScansOnDevice& dev, int S, int R, float* gap) {
	if (n) hipLaunchKernelGGL(dvp_cs_gaps, grid_of((size_t)n), dim3(256), 0, st, xyz, (uint32_t)n, dev.records(), S, R, dev.map_bits(), dev.words, gap);
}

}   // namespace

extern "C" int dvp_cloud_scan_gaps(int device, const dvp_cloud_scan* scans, int num_scans, int cube_size, const float* query_xyz, long long num_query, float* gap_out, float* maps_out,
                                   float* truth_xyz_out) {
	const char* who = "dvp_cloud_scan_gaps";
	t_scan_error.clear();
	std::vector<Scan> list;
	long long total = 0;
	const std::string what = scans_of(scans, num_scans, cube_size, &list, &total);
	if (!what.empty()) return scan_fail(who, what);
	if (num_query < 0 || num_query > dvpce::kMaxPoints) return scan_fail(who, "a cloud holds 0 ... 2^31 - 1 points, got " + std::to_string(num_query));
	if (num_query > 0 && !query_xyz) return scan_fail(who, "the point arrays are required");
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return scan_fail(who, "hipSetDevice failed"); }
	ScansOnDevice dev;
	dvpmem::DevBlock queries;
	dvpmem::StreamScope st;
	if (st.open()) return scan_fail(who, "hipStreamCreate failed");
	Laps laps;
	const std::string made = splat_scans(st, list, total, cube_size, &dev, &laps);
	if (!made.empty()) return scan_fail(who, made);
	dvpmem::Carve carve;
	const size_t o_xyz = carve.take((size_t)num_query * 12), o_gap = carve.take((size_t)num_query * 4);
	if (queries.reserve(carve.total)) return scan_fail(who, out_of_memory(carve.total));
	uint8_t* q = queries.as<uint8_t>();
	bool ok = !num_query || hipMemcpyAsync(q + o_xyz, query_xyz, (size_t)num_query * 12, hipMemcpyHostToDevice, st) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); return scan_fail(who, "upload failed"); }
	laps.lap(st, "upload of the queries");
	launch_gaps(st, (const float*)(q + o_xyz), num_query, dev, num_scans, cube_size, (float*)(q + o_gap));
	laps.lap(st, "gaps");
	ok = hipGetLastError() == hipSuccess;
	if (ok && gap_out && num_query) ok = hipMemcpyAsync(gap_out, q + o_gap, (size_t)num_query * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
	if (ok && maps_out) ok = hipMemcpyAsync(maps_out, dev.maps.as<uint8_t>(), (size_t)num_scans * dev.words * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
	if (ok && truth_xyz_out && total) ok = hipMemcpyAsync(truth_xyz_out, dev.truth.as<uint8_t>(), (size_t)total * 12, hipMemcpyDeviceToHost, st) == hipSuccess;
	if (!ok || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return scan_fail(who, "the gaps could not be made or fetched"); }
	laps.lap(st, "read-back");
	if (laps.on) fprintf(stderr, "%s timing (%d scans, %lld points, cube %d, %lld queries):%s\n", who, num_scans, total, cube_size, num_query, laps.report.c_str());
	return 0;
}

extern "C" int dvp_cloud_evaluate_scans(int device, const float* recon_xyz, long long num_recon, const dvp_cloud_prep* prep_recon, const dvp_cloud_scan* scans, int num_scans,
                                        const dvp_cloud_prep* prep_truth, int cube_size, const float* tolerances, int num_tol, long long* within_recon, long long* within_truth,
                                        long long* used, long long* free_space, long long* counts_out, float* d2_recon_out, float* gap_out) {
	const char* who = "dvp_cloud_evaluate_scans";
	t_scan_error.clear();
	if (!within_recon || !within_truth || !used || !free_space || !counts_out) return scan_fail(who, "within_recon, within_truth, used, free_space and counts_out are required");
	if (!tolerances) return scan_fail(who, "the tolerances are required");
	std::string what = dvpce::check_tolerances(tolerances, num_tol);
	if (!what.empty()) return scan_fail(who, what);
	std::vector<Scan> list;
	long long total = 0;
	what = scans_of(scans, num_scans, cube_size, &list, &total);
	if (!what.empty()) return scan_fail(who, what);
	if (num_recon < 0 || num_recon > dvpce::kMaxPoints) return scan_fail(who, "a cloud holds 0 ... 2^31 - 1 points, got " + std::to_string(num_recon));
	if (num_recon > 0 && !recon_xyz) return scan_fail(who, "the point arrays are required");
	dvpcp::Prep prep[2];
	const dvp_cloud_prep* const given[2] = { prep_recon, prep_truth };
	for (int c = 0; c < 2; ++c) {
		if (!given[c]) continue;
		what = dvpcp::prep_of_abi(given[c], &prep[c]);
		if (!what.empty()) return scan_fail(who, what);
	}
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return scan_fail(who, "hipSetDevice failed"); }
	ScansOnDevice dev;
	dvpcp::ResidentCloud cloud[2];
	dvpmem::DevBlock raw, side;
	dvpmem::StreamScope st;
	if (st.open()) return scan_fail(who, "hipStreamCreate failed");
	Laps laps;
	what = splat_scans(st, list, total, cube_size, &dev, &laps);
	if (!what.empty()) return scan_fail(who, what);
	// both clouds prepared where they lie; the raw ones go as soon as they are
	if (raw.reserve((size_t)num_recon * 12)) return scan_fail(who, out_of_memory((size_t)num_recon * 12));
	if (num_recon && (hipMemcpyAsync(raw.as<float>(), recon_xyz, (size_t)num_recon * 12, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
		(void)hipGetLastError();
		return scan_fail(who, "upload failed");
	}
	laps.lap(st, "upload of the reconstruction");
	what = dvpcp::prepare_resident(st, raw.as<float>(), num_recon, prep[0], &cloud[0]);
	raw.release();
	if (what.empty()) what = dvpcp::prepare_resident(st, dev.truth.as<float>(), total, prep[1], &cloud[1]);
	dev.truth.release();
	if (!what.empty()) return scan_fail(who, what);
	laps.lap(st, "prepare");
	for (int c = 0; c < 2; ++c)
		for (int k = 0; k < 4; ++k) counts_out[4 * c + k] = cloud[c].counts[k];
	const long long n = cloud[0].num;
	dvpmem::Carve carve;
	const size_t o_d2 = carve.take((size_t)n * 4), o_gap = carve.take((size_t)n * 4), o_free = carve.take(dvpce::kMaxTolerances * 8);
	if (side.reserve(carve.total)) return scan_fail(who, out_of_memory(carve.total));
	uint8_t* b = side.as<uint8_t>();
	if (laps.on) fprintf(stderr, "%s timing (%d scans, %lld points, cube %d, %lld + %lld prepared):%s\n", who, num_scans, total, cube_size, n, cloud[1].num, laps.report.c_str());
	laps.report.clear();
	const float* const dev_xyz[2] = { cloud[0].xyz(), cloud[1].xyz() };
	const long long num_out[2] = { cloud[0].num, cloud[1].num };
	const dvpce::Bounds bounds[2] = { cloud[0].bounds, cloud[1].bounds };
	long long* const within[2] = { within_recon, within_truth };
	float* const d2[2] = { d2_recon_out, nullptr };
	if (dvpce::cloud_run_on_device(who, device, dev_xyz, num_out, bounds, tolerances, num_tol, within, used, d2, (float*)(b + o_d2)) != 0) {
		t_scan_error.text = dvp_cloud_last_error();
		return 1;
	}
	laps.last = std::chrono::steady_clock::now();
	Tolerances tol;
	tol.count = num_tol;
	for (int k = 0; k < dvpce::kMaxTolerances; ++k) {
		tol.t[k] = k < num_tol ? tolerances[k] : 0.0f;
		tol.t2[k] = tol.t[k] * tol.t[k];
	}
	if (hipMemsetAsync(b + o_free, 0, dvpce::kMaxTolerances * 8, st) != hipSuccess) { (void)hipGetLastError(); return scan_fail(who, "the counts could not be cleared"); }
	launch_gaps(st, cloud[0].xyz(), n, dev, num_scans, cube_size, (float*)(b + o_gap));
	laps.lap(st, "gaps");
	if (n) hipLaunchKernelGGL(dvp_cs_count, grid_of((size_t)n), dim3(256), 0, st, (const float*)(b + o_d2), (const float*)(b + o_gap), (uint32_t)n, tol, (unsigned long long*)(b + o_free));
	laps.lap(st, "count");
	unsigned long long host_free[dvpce::kMaxTolerances];
	bool ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(host_free, b + o_free, sizeof host_free, hipMemcpyDeviceToHost, st) == hipSuccess;
	if (ok && gap_out && n) ok = hipMemcpyAsync(gap_out, b + o_gap, (size_t)n * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
	if (!ok || hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return scan_fail(who, "the gaps could not be made or fetched"); }
	laps.lap(st, "read-back");
	for (int k = 0; k < num_tol; ++k) free_space[k] = (long long)host_free[k];
	if (laps.on) fprintf(stderr, "%s timing, after the distances:%s\n", who, laps.report.c_str());
	return 0;
}
