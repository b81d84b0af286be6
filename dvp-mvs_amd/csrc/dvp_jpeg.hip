// dvp_jpeg.hip — baseline JPEG on the device (what the reference's cv::imwrite of its preview images writes, APD.cpp:694-812,
// main.cpp:219-223, 383-403) and the preview renderers.  The arithmetic lives in dvp_jpeg.hpp; this file maps it onto the GPU:
//   1. dvp_jpeg_coefs_*: a lane per MCU — colour conversion, down-sampling, FDCT, quantisation -> zig-zag int16 + a mask of
//      the non-zero coefficients;
//   2. dvp_jpeg_seg_size: a lane per restart segment — the segment's byte length (Huffman bits, 1-bit padding, FF 00
//      stuffing, RST marker) by running the coder with a counting sink;
//   3. dvp_jpeg_scan: the exclusive scan of those lengths (one work-group); the host reads the total (its one sync);
//   4. dvp_jpeg_seg_write: a lane per segment codes it again, straight to its final offset.
// Restart intervals make the segments independent: each starts on a byte boundary with DC predictions of 0.
#include <hip/hip_runtime.h>

#include <string.h>

#include <string>

#include "../../include/dvp_mvs.h"
#include "dvp_jpeg_enc.h"

namespace dvpjpeg {

__global__ void __launch_bounds__(256) dvp_jpeg_coefs_color(const uint8_t* __restrict__ pix, long long pitch, int W, int H, int mcx, long long nmcu,
                                                            const Tables* __restrict__ t, int16_t* __restrict__ coef, uint64_t* __restrict__ mask) {
	const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (m >= nmcu) return;
	mcu_color(pix, pitch, W, H, (int)(m % mcx), (int)(m / mcx), t, coef + m * 384, mask + m * 6);
}

__global__ void __launch_bounds__(256) dvp_jpeg_coefs_grey(const uint8_t* __restrict__ pix, long long pitch, int W, int H, int mcx, long long nmcu,
                                                           const Tables* __restrict__ t, int16_t* __restrict__ coef, uint64_t* __restrict__ mask) {
	const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (m >= nmcu) return;
	mcu_grey(pix, pitch, W, H, (int)(m % mcx), (int)(m / mcx), t, coef + m * 64, mask + m);
}

__global__ void __launch_bounds__(64) dvp_jpeg_seg_size(const Tables* __restrict__ t, const int16_t* __restrict__ coef, const uint64_t* __restrict__ mask,
                                                        long long nmcu, int bpm, int R, long long nseg, unsigned* __restrict__ seglen) {
	const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg) return;
	const long long first = s * R, n = first + R <= nmcu ? R : nmcu - first;
	CountOut cnt;
	code_segment(t, coef, mask, first, n, bpm, cnt);
	seglen[s] = (unsigned)cnt.n + (s + 1 < nseg ? 2u : 0u);
}

// exclusive scan of n lengths by one work-group of 1024 lanes: each lane sums a run of consecutive entries, the run sums are
// scanned in LDS, then each lane writes its run's offsets; off[n] = total
__global__ void __launch_bounds__(1024) dvp_jpeg_scan(const unsigned* __restrict__ len, long long n, unsigned long long* __restrict__ off) {
	__shared__ unsigned long long part[1024];
	const int tid = threadIdx.x;
	const long long per = (n + 1023) / 1024, b0 = tid * per, b1 = b0 + per < n ? b0 + per : n;
	unsigned long long sum = 0;
	for (long long i = b0; i < b1; ++i) sum += len[i];
	part[tid] = sum;
	__syncthreads();
	for (int d = 1; d < 1024; d <<= 1) {
		const unsigned long long v = tid >= d ? part[tid - d] : 0ull;
		__syncthreads();
		part[tid] += v;
		__syncthreads();
	}
	unsigned long long acc = part[tid] - sum;
	for (long long i = b0; i < b1; ++i) { off[i] = acc; acc += len[i]; }
	if (tid == 1023) off[n] = part[1023];
}

__global__ void __launch_bounds__(64) dvp_jpeg_seg_write(const Tables* __restrict__ t, const int16_t* __restrict__ coef, const uint64_t* __restrict__ mask,
                                                         long long nmcu, int bpm, int R, long long nseg, const unsigned long long* __restrict__ off,
                                                         uint8_t* __restrict__ out) {
	const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= nseg) return;
	const long long first = s * R, n = first + R <= nmcu ? R : nmcu - first;
	WriteOut w{ out + off[s] };
	code_segment(t, coef, mask, first, n, bpm, w);
	if (s + 1 < nseg) { w.put(0xFF); w.put((uint8_t)(0xD0 + (s & 7))); }   // RST0..7 in turn (jcmarker.c emit_restart)
}

__global__ void __launch_bounds__(256) dvp_preview_render(const float4* __restrict__ planes, const uint8_t* __restrict__ weak, size_t L, float dmin, float dmax,
                                                          uint8_t* __restrict__ depth_bgr, uint8_t* __restrict__ normal_bgr, uint8_t* __restrict__ weak_bgr) {
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= L) return;
	const float4 ph = planes[i];
	const bool usable = !(ph.w < dmin || ph.w > dmax);   // the driver's unpack (main.cpp:300-309, dvp_unpack_maps)
	uint8_t o[3];
	if (depth_bgr) { render_depth(usable ? ph.w : 0.0f, dmin, dmax, o); depth_bgr[3 * i] = o[0]; depth_bgr[3 * i + 1] = o[1]; depth_bgr[3 * i + 2] = o[2]; }
	if (normal_bgr) { render_normal(ph.x, ph.y, ph.z, o); normal_bgr[3 * i] = o[0]; normal_bgr[3 * i + 1] = o[1]; normal_bgr[3 * i + 2] = o[2]; }
	if (weak_bgr) { render_weak(usable ? weak[i] : (uint8_t)DVP_UNKNOWN, o); weak_bgr[3 * i] = o[0]; weak_bgr[3 * i + 1] = o[1]; weak_bgr[3 * i + 2] = o[2]; }
}

int launch_render(hipStream_t stream, const float* planes, const uint8_t* weak, size_t L, float dmin, float dmax,
                  uint8_t* depth_bgr, uint8_t* normal_bgr, uint8_t* weak_bgr) {
	if (!L) return 0;
	hipLaunchKernelGGL(dvp_preview_render, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const float4*>(planes), weak, L,
	                   dmin, dmax, depth_bgr, normal_bgr, weak_bgr);
	return hipGetLastError() != hipSuccess;
}

// Colour: 8 MCUs (2048 pixels) per segment, grey: 32 blocks (the same pixels).  A lane of steps 2 and 4 codes a segment
// serially, so R sets their latency whatever the image size (measured: R = 32 took 12-13 ms for the three previews of a view at
// both 6 and 25 Mpx); a segment costs 3-4 bytes of marker, padding and fresh DC predictions (R = 32: +0.1-0.6 % file size,
// profiles/preview_jpeg.txt has R = 8).
int default_restart(int channels) { return channels == 3 ? 8 : 32; }

int encode_begin(Encoder& e, hipStream_t stream, const uint8_t* pixels, long long pitch, int W, int H, int C, int quality, int restart,
                 unsigned long long* total_host) {
	e.error = nullptr;
	if (W < 1 || H < 1 || W > 65535 || H > 65535 || (C != 1 && C != 3) || pitch < (long long)W * C) { e.error = "jpeg: bad image geometry"; return 1; }
	if (quality < 1 || quality > 100) { e.error = "jpeg: quality must be 1..100"; return 1; }
	if (restart < 0 || restart > 65535) { e.error = "jpeg: restart interval must be 0..65535"; return 1; }
	e.W = W; e.H = H; e.C = C;
	e.R = restart ? restart : default_restart(C);
	e.bpm = C == 3 ? 6 : 1;
	const long long mcx = C == 3 ? (W + 15) / 16 : (W + 7) / 8, mcy = C == 3 ? (H + 15) / 16 : (H + 7) / 8;
	e.nmcu = mcx * mcy;
	e.nseg = (e.nmcu + e.R - 1) / e.R;
	build_tables(quality, &e.tab);
	e.header_len = build_header(&e.tab, W, H, C, e.R, e.header);
	const size_t blocks = (size_t)e.nmcu * e.bpm, segs = (size_t)e.nseg + 1;
	if (e.d_tab.reserve(sizeof(Tables)) || e.coef.reserve(blocks * 64 * sizeof(int16_t)) || e.mask.reserve(blocks * sizeof(uint64_t)) ||
	    e.seglen.reserve(segs * sizeof(unsigned)) || e.segoff.reserve(segs * sizeof(unsigned long long))) { e.error = "jpeg: out of device memory"; return 1; }
	Tables* d_tab = e.d_tab.as<Tables>(); int16_t* coef = e.coef.as<int16_t>();
	uint64_t* mask = e.mask.as<uint64_t>();
	unsigned* seglen = e.seglen.as<unsigned>(); unsigned long long* segoff = e.segoff.as<unsigned long long>();
	if (hipMemcpyAsync(d_tab, &e.tab, sizeof(Tables), hipMemcpyHostToDevice, stream) != hipSuccess) { e.error = "jpeg: table upload failed"; return 1; }
	const unsigned g1 = (unsigned)((e.nmcu + 255) / 256), g2 = (unsigned)((e.nseg + 63) / 64);
	if (C == 3) hipLaunchKernelGGL(dvp_jpeg_coefs_color, dim3(g1), dim3(256), 0, stream, pixels, pitch, W, H, (int)mcx, e.nmcu, d_tab, coef, mask);
	else hipLaunchKernelGGL(dvp_jpeg_coefs_grey, dim3(g1), dim3(256), 0, stream, pixels, pitch, W, H, (int)mcx, e.nmcu, d_tab, coef, mask);
	hipLaunchKernelGGL(dvp_jpeg_seg_size, dim3(g2), dim3(64), 0, stream, d_tab, coef, mask, e.nmcu, e.bpm, e.R, e.nseg, seglen);
	hipLaunchKernelGGL(dvp_jpeg_scan, dim3(1), dim3(1024), 0, stream, seglen, e.nseg, segoff);
	if (hipGetLastError() != hipSuccess) { e.error = "jpeg: launch failed"; return 1; }
	if (hipMemcpyAsync(total_host, segoff + e.nseg, 8, hipMemcpyDeviceToHost, stream) != hipSuccess) { e.error = "jpeg: size read-back failed"; return 1; }
	return 0;
}

int encode_write(Encoder& e, hipStream_t stream, unsigned long long total) {
	e.error = nullptr;
	if (e.out.reserve(total ? (size_t)total : 1)) { e.error = "jpeg: out of device memory"; return 1; }
	e.data_bytes = total;
	hipLaunchKernelGGL(dvp_jpeg_seg_write, dim3((unsigned)((e.nseg + 63) / 64)), dim3(64), 0, stream, e.d_tab.as<Tables>(), e.coef.as<int16_t>(),
	                   e.mask.as<uint64_t>(), e.nmcu, e.bpm, e.R, e.nseg, e.segoff.as<unsigned long long>(), e.out.as<uint8_t>());
	if (hipGetLastError() != hipSuccess) { e.error = "jpeg: launch failed"; return 1; }
	return 0;
}

}   // namespace dvpjpeg

static thread_local dvpmem::CallError t_jpeg_error;

extern "C" const char* dvp_jpeg_last_error(void) { return t_jpeg_error.c_str(); }

extern "C" long long dvp_jpeg_bound(int width, int height, int channels) {
	if (width < 1 || height < 1 || (channels != 1 && channels != 3)) return -1;
	// per block at most 11 + 11 DC bits and 63 x (16 + 10) AC bits = 208 bytes, doubled for FF 00 stuffing; per MCU at most a
	// padding byte (stuffed) and an RST marker; the header is under 1024 bytes
	const long long bx = (width + 15) / 16 * 2, by = (height + 15) / 16 * 2;
	return 1024 + bx * by * 416 + bx * by * 4 + 2;
}

extern "C" int dvp_jpeg_encode(int device, const uint8_t* pixels, int width, int height, int channels, long long pitch_bytes, int quality,
                               int restart_mcus, uint8_t* dst, long long capacity, long long* bytes) {
	t_jpeg_error.clear();
	auto fail = [](const char* what) { return t_jpeg_error.fail(nullptr, what); };   // (the messages name the call themselves)
	if (!pixels || !bytes) return fail("dvp_jpeg_encode: pixels and bytes are required");
	if (width < 1 || height < 1 || (channels != 1 && channels != 3) || pitch_bytes < (long long)width * channels) return fail("dvp_jpeg_encode: bad image geometry");
	if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return fail("dvp_jpeg_encode: hipSetDevice failed"); }
	struct Pinned { unsigned long long* p = nullptr; ~Pinned() { if (p) (void)hipHostFree(p); } } total;   // the data size, copied on the stream
	dvpjpeg::Encoder e;
	dvpmem::DevBlock d_pix;
	dvpmem::StreamScope s;
	if (s.open()) return fail("dvp_jpeg_encode: hipStreamCreate failed");
	const size_t row = (size_t)width * channels;
	if (hipHostMalloc(reinterpret_cast<void**>(&total.p), 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); total.p = nullptr; return fail("dvp_jpeg_encode: out of host memory"); }
	if (d_pix.reserve(row * height)) return fail("dvp_jpeg_encode: out of device memory");
	if (hipMemcpy2DAsync(d_pix.as<uint8_t>(), row, pixels, (size_t)pitch_bytes, row, height, hipMemcpyHostToDevice, s) != hipSuccess) return fail("dvp_jpeg_encode: upload failed");
	if (dvpjpeg::encode_begin(e, s, d_pix.as<uint8_t>(), (long long)row, width, height, channels, quality, restart_mcus, total.p) ||
	    hipStreamSynchronize(s) != hipSuccess || dvpjpeg::encode_write(e, s, *total.p)) return fail(e.error ? e.error : "dvp_jpeg_encode: device step failed");
	*bytes = (long long)dvpjpeg::file_bytes(e);
	if (!dst || capacity < *bytes) return fail("dvp_jpeg_encode: capacity below the encoded size (*bytes)");
	memcpy(dst, e.header, e.header_len);
	if (hipMemcpyAsync(dst + e.header_len, e.out.as<uint8_t>(), e.data_bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("dvp_jpeg_encode: download failed");
	dst[*bytes - 2] = 0xFF;
	dst[*bytes - 1] = 0xD9;
	return 0;
}
