// dvp_jpeg_dec.hip — the input JPEGs reconstructed on the device (`apd --decode-on gpu`): the counterpart of dvp_jpeg.hip, which
// encodes.  The marker parse and the Huffman decode are sequential and stay on the host (dvp_jpeg_dec_mid.hpp, the text the host
// mirror's DecodeJpeg runs); they leave coefficient records per component.  What is independent per block and per pixel runs here,
// with the arithmetic of dvp_jpeg_dec.hpp:
//   dvp_jd_blocks   one launch per component: records -> dequantised coefficients -> inverse DCT -> clamp -> the component's plane.
//                   Eight lanes own an 8 x 8 block, a wave eight blocks that follow each other in the component's raster order,
//                   a work-group 32.  The block's coefficients are scattered into LDS (zero-filled first), lane j transforms
//                   column j in place, then row j, and stores its eight bytes at once: a wave writes eight pieces of 64
//                   contiguous bytes.  LDS layout: rows of 9 words, blocks of 72 — the column pass touches word 8 b + 9 r + j
//                   (r fixed per instruction), the row pass word 8 b + 9 j + c (c fixed): both hit every bank once per 32 lanes,
//                   modulo 32 banks as well as modulo 64.
//   dvp_jd_colour   three channels only: a lane per pixel, a work-group 256 pixels of one row; B, G, R are staged in LDS and the
//                   768 bytes leave in three coalesced byte stores per lane.
// The grey plane is written at the image's own pitch with the blocks beyond the right and bottom edge clipped — straight into the
// image store's slot for dvp_jpeg_decode_into_store; the component planes of the colour path are padded to whole MCUs, the colour launch
// reads the image's part of them.  Indices inside a plane are 32-bit: padded width x padded height < 2^31 is checked.
// Device memory: one DevBlock per call, carved; the stream of a call is a StreamScope.
// With dvp_jpeg_set_entropy(1) (`apd --entropy-on gpu`) the Huffman decode moves to the device as well: the headers are parsed here,
// the file's entropy-coded bytes go up instead of records, dvp_jpeg_huff.hip makes the records in device memory — they never exist on
// the host — and the two launches above read them unchanged.  A file the device path does not take (fill bytes, stray markers, a
// raised flag, the round cap, a refused allocation) goes through Decoder::decode as if the switch were off: a rejected file carries
// the serial scan's message, an accepted one the serial scan's records.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_devmem.hpp"
#include "dvp_jpeg_dec.hpp"
#include "dvp_jpeg_dec_mid.hpp"
#include "dvp_jpeg_huff_run.h"
#include "dvp_pyramid_run.h"

#include <atomic>
#include <vector>

namespace dvpjd {

constexpr int kGroupBlocks = 32;               // 8 x 8 blocks per work-group: 256 lanes
constexpr int kRowWords = 9, kBlockWords = 72;

__global__ void __launch_bounds__(256) dvp_jd_blocks(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ records, const QTable qt, unsigned blocks, int blocks_w,
                                                     uint8_t* __restrict__ out, size_t pitch, int clip_w, int clip_h) {
	__shared__ int ws[kGroupBlocks * kBlockWords];
	__shared__ uint16_t q[64];
	const int t = threadIdx.x, slot = t >> 3, j = t & 7;
	if (t < 64) q[t] = qt.q[t];
	int* w = ws + slot * kBlockWords;
	for (int k = j; k < kBlockWords; k += 8) w[k] = 0;
	__syncthreads();
	const unsigned g = blockIdx.x * (unsigned)kGroupBlocks + (unsigned)slot;
	const bool live = g < blocks;   // (the lanes of a slot past the last block go through the passes on zeros: every lane meets every barrier)
	if (live) {
		const uint32_t end = offsets[g + 1];
		for (uint32_t k = offsets[g] + (uint32_t)j; k < end; k += 8) {
			const uint32_t rec = records[k];
			const int pos = record_position(rec);
			w[(pos >> 3) * kRowWords + (pos & 7)] = dequantised(rec, q);
		}
	}
	__syncthreads();
	idct_column(w, w, kRowWords, j);
	__syncthreads();
	uint8_t px[8];
	idct_row(w, kRowWords, j, px);
	if (!live) return;
	const int X = (int)(g % (unsigned)blocks_w) * 8, Y = (int)(g / (unsigned)blocks_w) * 8 + j;
	if (X >= clip_w || Y >= clip_h) return;
	uint8_t* o = out + (size_t)Y * pitch + (size_t)X;
	if (X + 8 <= clip_w && ((uintptr_t)o & 7) == 0) {
		uint2 v;
		v.x = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
		v.y = (uint32_t)px[4] | ((uint32_t)px[5] << 8) | ((uint32_t)px[6] << 16) | ((uint32_t)px[7] << 24);
		*reinterpret_cast<uint2*>(o) = v;
	} else {
		for (int c = 0; c < 8 && X + c < clip_w; ++c) o[c] = px[c];
	}
}

struct PlaneRef {
	const uint8_t* p;   // blocks_w * 8 bytes per row
	int pitch, h, v;
};

// comps = 1: grey in three channels
__global__ void __launch_bounds__(256) dvp_jd_colour(const PlaneRef Yp, const PlaneRef Cb, const PlaneRef Cr, int comps, int hmax, int vmax, int width, uint8_t* __restrict__ out,
                                                     size_t pitch) {
	__shared__ uint8_t row[768];
	const int t = threadIdx.x, x0 = blockIdx.x * 256, x = x0 + t, y = blockIdx.y;
	if (x < width) {
		const int yy = Yp.p[(size_t)sample_row(y, Yp.v, vmax) * Yp.pitch + sample_col(x, Yp.h, hmax)];
		uint8_t bgr[3] = { (uint8_t)yy, (uint8_t)yy, (uint8_t)yy };
		if (comps == 3)
			ycc_to_bgr(yy, Cb.p[(size_t)sample_row(y, Cb.v, vmax) * Cb.pitch + sample_col(x, Cb.h, hmax)], Cr.p[(size_t)sample_row(y, Cr.v, vmax) * Cr.pitch + sample_col(x, Cr.h, hmax)], bgr);
		row[3 * t] = bgr[0];
		row[3 * t + 1] = bgr[1];
		row[3 * t + 2] = bgr[2];
	}
	__syncthreads();
	const int n = 3 * (width - x0 < 256 ? width - x0 : 256);
	uint8_t* o = out + (size_t)y * pitch + (size_t)x0 * 3;
	for (int k = t; k < n; k += 256) o[k] = row[k];
}

}   // namespace dvpjd

using dvpjdmid::Component;
using dvpjdmid::Decoder;

static thread_local dvpmem::CallError t_jd_error;
static thread_local double t_jd_ms[2] = { 0, 0 };
static thread_local long long t_jd_counts[2] = { 0, 0 };
static thread_local dvpjh::ScanStats t_je_stats;
static std::atomic<int> g_entropy_on_device{ 0 };
static int jd_fail(const char* who, const std::string& what) { return t_jd_error.fail(who, what); }

extern "C" void dvp_jpeg_set_entropy(int on_device) { g_entropy_on_device.store(on_device ? 1 : 0); }

extern "C" int dvp_jpeg_entropy_stats(long long* counts) {
	if (!counts) return 1;
	const dvpjh::ScanStats& s = t_je_stats;
	const long long v[8] = { s.path, s.segments, s.subsequences, s.chunks, s.longest, s.rounds, s.uploaded, s.decodes };
	for (int k = 0; k < 8; ++k) counts[k] = v[k];
	return 0;
}

extern "C" int dvp_jpeg_entropy_phases(double* ms) {
	if (!ms) return 1;
	for (int k = 0; k < dvpjh::kMsPhases; ++k) ms[k] = t_je_stats.ms[k];
	return 0;
}

extern "C" const char* dvp_jpeg_decode_last_error(void) { return t_jd_error.c_str(); }

extern "C" int dvp_jpeg_decode_timings(double* ms, long long* counts) {
	if (ms) { ms[0] = t_jd_ms[0]; ms[1] = t_jd_ms[1]; }
	if (counts) { counts[0] = t_jd_counts[0]; counts[1] = t_jd_counts[1]; }
	return 0;
}

namespace {

using clock_type = std::chrono::steady_clock;
double ms_since(clock_type::time_point t0) { return std::chrono::duration<double, std::milli>(clock_type::now() - t0).count(); }

// the largest component plane: the image padded to whole MCUs
bool planes_fit(const Decoder& d) {
	const long long pw = (long long)((d.width + 8 * d.hmax - 1) / (8 * d.hmax)) * 8 * d.hmax, ph = (long long)((d.height + 8 * d.vmax - 1) / (8 * d.vmax)) * 8 * d.vmax;
	return pw * ph < 0x80000000LL;
}

// The device half of a decode on `st`: the wanted components' records go up into `pool` (grown as needed), one dvp_jd_blocks per
// component, and for three channels dvp_jd_colour.  channels 1: the luma plane to dst at dst_pitch, clipped to width x height;
// 3: B, G, R.  dst is device memory, or NULL: then the result is made in the pool and *made points at it (pitch width * channels).
// No wait.  NULL = done, else what failed.
// `on_device`: the records are in device memory already (dvp_jpeg_huff.hip made them) and nothing is uploaded.
const char* reconstruct_on_device(const Decoder& d, int channels, hipStream_t st, dvpmem::DevBlock& pool, uint8_t* dst, size_t dst_pitch, uint8_t** made, const dvpjh::DeviceScan* on_device = nullptr) {
	const int n = channels == 1 ? 1 : (int)d.comps.size();
	dvpmem::Carve c;
	size_t o_offsets[3] = { 0, 0, 0 }, o_records[3] = { 0, 0, 0 }, o_plane[3] = { 0, 0, 0 };
	for (int i = 0; i < n; ++i) {
		const Component& k = d.comps[i];
		if (!on_device) {
			o_offsets[i] = c.take(k.offsets.size() * 4);
			o_records[i] = c.take(k.records.size() * 4);
		}
		if (channels == 3) o_plane[i] = c.take((size_t)k.blocks_w * 8 * k.blocks_h * 8);
	}
	const size_t o_dst = dst ? 0 : c.take((size_t)d.width * channels * d.height);
	if (pool.reserve(c.total, st)) return "out of device memory";
	uint8_t* base = pool.as<uint8_t>();
	if (!dst) { dst = base + o_dst; dst_pitch = (size_t)d.width * channels; }
	if (made) *made = dst;
	dvpjd::PlaneRef planes[3] = { { nullptr, 0, 1, 1 }, { nullptr, 0, 1, 1 }, { nullptr, 0, 1, 1 } };
	for (int i = 0; i < n; ++i) {
		const Component& k = d.comps[i];
		if (!on_device && (hipMemcpyAsync(base + o_offsets[i], k.offsets.data(), k.offsets.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
		                   hipMemcpyAsync(base + o_records[i], k.records.data(), k.records.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess)) {
			(void)hipGetLastError();
			return "upload failed";
		}
		const uint32_t* offsets = on_device ? on_device->offsets[i] : (const uint32_t*)(base + o_offsets[i]);
		const uint32_t* records = on_device ? on_device->records[i] : (const uint32_t*)(base + o_records[i]);
		dvpjd::QTable qt;
		for (int z = 0; z < 64; ++z) qt.q[z] = d.qt[k.tq][z];
		const unsigned blocks = (unsigned)((size_t)k.blocks_w * k.blocks_h);
		const unsigned groups = (blocks + dvpjd::kGroupBlocks - 1) / dvpjd::kGroupBlocks;
		const int pw = k.blocks_w * 8, ph = k.blocks_h * 8;
		if (channels == 1)
			hipLaunchKernelGGL(dvpjd::dvp_jd_blocks, dim3(groups), dim3(256), 0, st, offsets, records, qt, blocks, k.blocks_w, dst, dst_pitch, d.width, d.height);
		else
			hipLaunchKernelGGL(dvpjd::dvp_jd_blocks, dim3(groups), dim3(256), 0, st, offsets, records, qt, blocks, k.blocks_w, base + o_plane[i], (size_t)pw, pw, ph);
		if (hipGetLastError() != hipSuccess) return "launch failed";
		planes[i] = dvpjd::PlaneRef{ base + o_plane[i], pw, k.h, k.v };
	}
	if (channels == 3) {
		hipLaunchKernelGGL(dvpjd::dvp_jd_colour, dim3((unsigned)((d.width + 255) / 256), (unsigned)d.height), dim3(256), 0, st, planes[0], planes[1], planes[2], n, d.hmax, d.vmax, d.width,
		                   dst, dst_pitch);
		if (hipGetLastError() != hipSuccess) return "launch failed";
	}
	return nullptr;
}

void note_counts(const Decoder& d, int channels) {
	long long bytes = 0, blocks = 0;
	for (size_t i = 0; i < (channels == 1 ? 1 : d.comps.size()); ++i) {
		bytes += (long long)(d.comps[i].offsets.size() + d.comps[i].records.size()) * 4;
		blocks += (long long)d.comps[i].blocks_w * d.comps[i].blocks_h;
	}
	t_jd_counts[0] = bytes;
	t_jd_counts[1] = blocks;
}

// A call's file from its bytes to its records.  With the entropy switch off, parse() is Decoder::decode and the records are on the
// host.  With it on, parse() stops before the scan and plans it (dvpjh::plan: the pre-scan); a file the plan does not take is
// decoded as if the switch were off.  records_on_device() then runs the planned scan on the call's stream and, when it gives up,
// runs Decoder::decode after all.  The blocks are members: declare a Scan BEFORE the call's StreamScope.
struct Scan {
	Decoder d;
	dvpjh::Plan plan;
	bool planned = false;
	dvpmem::DevBlock work, recs;
	dvpjh::DeviceScan on_device;
	const dvpjh::DeviceScan* records() const { return planned ? &on_device : nullptr; }

	bool parse(const uint8_t* file, size_t bytes, bool luma_only) {   // false: d.error
		t_je_stats = dvpjh::ScanStats();
		if (g_entropy_on_device.load() != 0) {
			const clock_type::time_point t0 = clock_type::now();
			d.stop_at_scan = true;
			if (!d.decode(file, bytes, luma_only)) return false;
			planned = dvpjh::plan(d, luma_only, dvpjh::subseq_bytes_in_use(), &plan);
			if (planned) { t_je_stats.ms[dvpjh::kMsPrescan] = ms_since(t0); return true; }
			d = Decoder();
		}
		return d.decode(file, bytes, luma_only);
	}
	// NULL, or the serial scan's message for a file it refuses
	const char* records_on_device(const uint8_t* file, size_t bytes, bool luma_only, hipStream_t st) {
		if (!planned) return nullptr;
		const char* why = "";
		if (dvpjh::scan_on_device(plan, dvpjh::subseq_bytes_in_use(), st, work, recs, &on_device, &t_je_stats, &why) == 0) {
			t_je_stats.path = dvpjh::kPathDevice;
			return nullptr;
		}
		t_je_stats.path = dvpjh::kPathFellBack;
		planned = false;
		work.release();
		recs.release();
		d = Decoder();
		return d.decode(file, bytes, luma_only) ? nullptr : d.error;
	}
	void note(int channels) const {
		if (!planned) { note_counts(d, channels); return; }
		long long words = 0, blocks = 0;
		for (size_t i = 0; i < (channels == 1 ? 1 : d.comps.size()); ++i) {
			words += (long long)(on_device.offset_words[i] + on_device.record_words[i]);
			blocks += (long long)d.comps[i].blocks_w * d.comps[i].blocks_h;
		}
		t_jd_counts[0] = words * 4;
		t_jd_counts[1] = blocks;
	}
};

// a serialised run books the reconstruction as the last phase
void book_reconstruction(hipStream_t st, clock_type::time_point since) {
	if (t_je_stats.path != dvpjh::kPathDevice || !dvpjh::serialised_run()) return;
	(void)hipStreamSynchronize(st);
	t_je_stats.ms[dvpjh::kMsReconstruct] = ms_since(since);
}

}   // namespace

extern "C" int dvp_jpeg_decode(int device, const uint8_t* file, long long file_bytes, int channels, uint8_t* out, long long pitch_bytes, int* width, int* height) {
	const char* who = "dvp_jpeg_decode";
	t_jd_error.clear();
	if (!file || file_bytes <= 0) return jd_fail(who, "the file's bytes are required");
	if (channels != 1 && channels != 3) return jd_fail(who, "channels must be 1 (luma) or 3 (B, G, R)");
	if (!out) {   // the size alone, from the frame header: nothing touches the device
		Decoder d;
		if (!d.decode(file, (size_t)file_bytes, channels == 1, true)) return jd_fail(who, d.error);
		if (width) *width = d.width;
		if (height) *height = d.height;
		return 0;
	}
	const clock_type::time_point t0 = clock_type::now();
	Scan scan;
	Decoder& d = scan.d;
	if (!scan.parse(file, (size_t)file_bytes, channels == 1)) return jd_fail(who, d.error);
	if (pitch_bytes < (long long)d.width * channels) return jd_fail(who, "the pitch is below width * channels bytes");
	if (!planes_fit(d)) return jd_fail(who, "the image is too large (padded width x padded height must stay below 2^31)");
	t_jd_ms[0] = ms_since(t0);
	const clock_type::time_point t1 = clock_type::now();
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return jd_fail(who, "hipSetDevice failed"); }
	dvpmem::DevBlock pool;
	dvpmem::StreamScope st;
	if (st.open()) return jd_fail(who, "hipStreamCreate failed");
	if (const char* refused = scan.records_on_device(file, (size_t)file_bytes, channels == 1, st)) return jd_fail(who, refused);
	scan.note(channels);
	const clock_type::time_point t2 = clock_type::now();
	uint8_t* made = nullptr;
	if (const char* what = reconstruct_on_device(d, channels, st, pool, nullptr, 0, &made, scan.records())) return jd_fail(who, what);
	book_reconstruction(st, t2);
	const size_t row = (size_t)d.width * channels;
	if (hipMemcpy2DAsync(out, (size_t)pitch_bytes, made, row, row, (size_t)d.height, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
		(void)hipGetLastError();
		return jd_fail(who, "the image could not be made or fetched");
	}
	t_jd_ms[1] = ms_since(t1);
	if (width) *width = d.width;
	if (height) *height = d.height;
	return 0;
}

extern "C" int dvp_jpeg_decode_into_store(dvp_images* store, int id, const uint8_t* file, long long file_bytes, uint8_t* grey_out_or_null, long long pitch_bytes) {
	const char* who = "dvp_jpeg_decode_into_store";
	t_jd_error.clear();
	if (!store) return jd_fail(who, "the store is required");
	if (!file || file_bytes <= 0) return jd_fail(who, "the file's bytes are required");
	if (dvppyr::store_has(store, id)) return jd_fail(who, "image id " + std::to_string(id) + " is already in the store");
	const clock_type::time_point t0 = clock_type::now();
	Scan scan;
	Decoder& d = scan.d;
	if (!scan.parse(file, (size_t)file_bytes, true)) return jd_fail(who, d.error);
	if (d.width > 32767 || d.height > 32767) return jd_fail(who, "bad image geometry (sizes of 1 ... 32767)");
	if (grey_out_or_null && pitch_bytes < d.width) return jd_fail(who, "the pitch is below the width");
	t_jd_ms[0] = ms_since(t0);
	const clock_type::time_point t1 = clock_type::now();
	if (hipSetDevice(dvppyr::store_device(store)) != hipSuccess) { (void)hipGetLastError(); return jd_fail(who, "hipSetDevice failed"); }
	dvpmem::DevBlock slot, pool;
	dvpmem::StreamScope st;
	if (slot.reserve((size_t)d.width * d.height)) return jd_fail(who, "out of device memory");
	if (st.open()) return jd_fail(who, "hipStreamCreate failed");
	if (const char* refused = scan.records_on_device(file, (size_t)file_bytes, true, st)) return jd_fail(who, refused);
	scan.note(1);
	const clock_type::time_point t2 = clock_type::now();
	if (const char* what = reconstruct_on_device(d, 1, st, pool, slot.as<uint8_t>(), (size_t)d.width, nullptr, scan.records())) return jd_fail(who, what);
	book_reconstruction(st, t2);
	if (grey_out_or_null && hipMemcpy2DAsync(grey_out_or_null, (size_t)pitch_bytes, slot.as<uint8_t>(), (size_t)d.width, (size_t)d.width, (size_t)d.height, hipMemcpyDeviceToHost, st) != hipSuccess) {
		(void)hipGetLastError();
		return jd_fail(who, "the plane could not be fetched");
	}
	if (hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return jd_fail(who, "the plane could not be made"); }
	t_jd_ms[1] = ms_since(t1);
	// the slot is complete: it joins the store (another thread may have put the same id meanwhile: then this one is dropped)
	if (dvppyr::store_adopt(store, id, slot, d.width, d.height)) return jd_fail(who, "image id " + std::to_string(id) + " is already in the store");
	return 0;
}

// the records of a file's scan, from the serial scan (on_device 0) or from the device path (1; a file it does not take comes from
// the serial scan, and dvp_jpeg_entropy_stats says so).  Size-then-fill: with offsets and records NULL only the word counts are
// written; else offsets[i] and records[i] receive offset_words[i] and record_words[i] words for every component with a count.
extern "C" int dvp_jpeg_scan_records(int device, const uint8_t* file, long long file_bytes, int luma_only, int on_device, int* components, long long* offset_words, long long* record_words,
                                     uint32_t** offsets, uint32_t** records) {
	const char* who = "dvp_jpeg_scan_records";
	t_jd_error.clear();
	if (!file || file_bytes <= 0) return jd_fail(who, "the file's bytes are required");
	if (!components || !offset_words || !record_words) return jd_fail(who, "components, offset_words and record_words are required");
	if ((offsets == nullptr) != (records == nullptr)) return jd_fail(who, "offsets and records go together");
	t_je_stats = dvpjh::ScanStats();
	Decoder d;
	dvpjh::Plan plan;
	dvpmem::DevBlock work, recs;
	dvpmem::StreamScope st;
	dvpjh::DeviceScan made;
	bool planned = false;
	if (on_device) {
		d.stop_at_scan = true;
		if (!d.decode(file, (size_t)file_bytes, luma_only != 0)) return jd_fail(who, d.error);
		planned = dvpjh::plan(d, luma_only != 0, dvpjh::subseq_bytes_in_use(), &plan);
		if (planned) {
			if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return jd_fail(who, "hipSetDevice failed"); }
			if (st.open()) return jd_fail(who, "hipStreamCreate failed");
			const char* why = "";
			planned = dvpjh::scan_on_device(plan, dvpjh::subseq_bytes_in_use(), st, work, recs, &made, &t_je_stats, &why) == 0;
			t_je_stats.path = planned ? dvpjh::kPathDevice : dvpjh::kPathFellBack;
		}
		if (!planned) d = Decoder();
	}
	if (!planned && !d.decode(file, (size_t)file_bytes, luma_only != 0)) return jd_fail(who, d.error);
	*components = (int)d.comps.size();
	for (int i = 0; i < 3; ++i) {
		const bool has = i < (int)d.comps.size();
		offset_words[i] = !has ? 0 : (planned ? (long long)made.offset_words[i] : (long long)d.comps[i].offsets.size());
		record_words[i] = !has ? 0 : (planned ? (long long)made.record_words[i] : (long long)d.comps[i].records.size());
	}
	if (!offsets) return 0;
	for (int i = 0; i < (int)d.comps.size(); ++i) {
		if (!offset_words[i]) continue;
		if (!offsets[i] || !records[i]) return jd_fail(who, "an output array is missing");
		if (planned) {
			if (hipMemcpyAsync(offsets[i], made.offsets[i], (size_t)offset_words[i] * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
			    hipMemcpyAsync(records[i], made.records[i], (size_t)record_words[i] * 4, hipMemcpyDeviceToHost, st) != hipSuccess) {
				(void)hipGetLastError();
				return jd_fail(who, "the records could not be fetched");
			}
		} else {
			std::copy(d.comps[i].offsets.begin(), d.comps[i].offsets.end(), offsets[i]);
			std::copy(d.comps[i].records.begin(), d.comps[i].records.end(), records[i]);
		}
	}
	if (planned && hipStreamSynchronize(st) != hipSuccess) { (void)hipGetLastError(); return jd_fail(who, "the records could not be fetched"); }
	return 0;
}
