// dvp_jpeg.hpp — the per-MCU and per-segment steps of the baseline JPEG encoder (csrc/dvp_jpeg.hip) and the preview
// renderers, written once for the device and the host (tests/jpeg_host builds the same steps serially for the CPU tests).
//
// What cv::imwrite asks libjpeg for, restated: quality scaling of the Annex K tables with force_baseline (jcparam.c),
// libjpeg's fixed-point RGB -> YCbCr (jccolor.c), h2v2 down-sampling with the alternating 1/2 bias and the right / bottom
// edges replicated to whole MCUs (jcsample.c, jcprepct.c), dummy blocks past the image's last block column / row that
// repeat the previous block's DC (jccoefct.c), the accurate integer FDCT (jfdctint.c), round-half-away quantisation
// (jcdctmgr.c) and the standard Huffman tables (jchuff.c) — plus a restart interval, so that every segment of R MCUs is
// byte-aligned and starts from a DC prediction of 0: the segments are coded in parallel.
#ifndef DVP_JPEG_HPP_
#define DVP_JPEG_HPP_

#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define DVP_JHD __host__ __device__ inline
#else
#define DVP_JHD inline
#endif

namespace dvpjpeg {

// Everything the coding steps look up, in one block of memory (device buffer on the GPU).
struct Tables {
	uint32_t dc[2][12];     // (code length << 16) | code, per DC category; [0] luminance, [1] chrominance
	uint32_t ac[2][256];    // the same per (run << 4 | size) symbol; 0 = symbol not in the table
	uint16_t qdiv[2][64];   // islow divisors (8 * quantiser), zig-zag order
	uint8_t natural[64];    // natural index of the k-th zig-zag coefficient (jpeg_natural_order)
	uint8_t qval[2][64];    // quantisers in zig-zag order, as the DQT segments carry them
};

DVP_JHD int imin(int a, int b) { return a < b ? a : b; }

// Samples of an 8x8 block, natural order, level-shifted; out: quantised coefficients in zig-zag order and the mask of the
// non-zero ones (bit k = zig-zag index k).
DVP_JHD uint64_t fdct_quant(int* d, const Tables* t, int tbl, int16_t* out) {
	const int CB = 13, PB = 2;
	// jfdctint.c (jpeg_fdct_islow), pass 1: rows
	for (int r = 0; r < 8; ++r) {
		int* p = d + 8 * r;
		const int tmp0 = p[0] + p[7], tmp7 = p[0] - p[7], tmp1 = p[1] + p[6], tmp6 = p[1] - p[6];
		const int tmp2 = p[2] + p[5], tmp5 = p[2] - p[5], tmp3 = p[3] + p[4], tmp4 = p[3] - p[4];
		const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
		p[0] = (tmp10 + tmp11) * (1 << PB);
		p[4] = (tmp10 - tmp11) * (1 << PB);
		int z1 = (tmp12 + tmp13) * 4433;
		p[2] = (z1 + tmp13 * 6270 + (1 << (CB - PB - 1))) >> (CB - PB);
		p[6] = (z1 + tmp12 * -15137 + (1 << (CB - PB - 1))) >> (CB - PB);
		z1 = tmp4 + tmp7;
		int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
		const int z5 = (z3 + z4) * 9633;
		const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
		z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
		z3 += z5; z4 += z5;
		p[7] = (t4 + z1 + z3 + (1 << (CB - PB - 1))) >> (CB - PB);
		p[5] = (t5 + z2 + z4 + (1 << (CB - PB - 1))) >> (CB - PB);
		p[3] = (t6 + z2 + z3 + (1 << (CB - PB - 1))) >> (CB - PB);
		p[1] = (t7 + z1 + z4 + (1 << (CB - PB - 1))) >> (CB - PB);
	}
	// pass 2: columns
	for (int c = 0; c < 8; ++c) {
		int* p = d + c;
		const int tmp0 = p[0] + p[56], tmp7 = p[0] - p[56], tmp1 = p[8] + p[48], tmp6 = p[8] - p[48];
		const int tmp2 = p[16] + p[40], tmp5 = p[16] - p[40], tmp3 = p[24] + p[32], tmp4 = p[24] - p[32];
		const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
		p[0] = (tmp10 + tmp11 + (1 << (PB - 1))) >> PB;
		p[32] = (tmp10 - tmp11 + (1 << (PB - 1))) >> PB;
		int z1 = (tmp12 + tmp13) * 4433;
		p[16] = (z1 + tmp13 * 6270 + (1 << (CB + PB - 1))) >> (CB + PB);
		p[48] = (z1 + tmp12 * -15137 + (1 << (CB + PB - 1))) >> (CB + PB);
		z1 = tmp4 + tmp7;
		int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
		const int z5 = (z3 + z4) * 9633;
		const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
		z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
		z3 += z5; z4 += z5;
		p[56] = (t4 + z1 + z3 + (1 << (CB + PB - 1))) >> (CB + PB);
		p[40] = (t5 + z2 + z4 + (1 << (CB + PB - 1))) >> (CB + PB);
		p[24] = (t6 + z2 + z3 + (1 << (CB + PB - 1))) >> (CB + PB);
		p[8] = (t7 + z1 + z4 + (1 << (CB + PB - 1))) >> (CB + PB);
	}
	// jcdctmgr.c quantize: (|x| + q/2) / q with the sign put back
	uint64_t mask = 0;
	for (int k = 0; k < 64; ++k) {
		const int x = d[t->natural[k]], q = t->qdiv[tbl][k];
		int v = ((x < 0 ? -x : x) + (q >> 1)) / q;
		if (x < 0) v = -v;
		out[k] = (int16_t)v;
		if (v) mask |= (uint64_t)1 << k;
	}
	return mask;
}

// One MCU of a 3-channel BGR image (4:2:0: Y00 Y01 Y10 Y11 Cb Cr).  pix: row-major bytes, `pitch` bytes per row.
DVP_JHD void ycc(const uint8_t* p, int& y, int& cb, int& cr) {
	const int b = p[0], g = p[1], r = p[2];   // jccolor.c rgb_ycc_convert, FIX(x) = x * 65536 rounded
	y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
	cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
	cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

DVP_JHD void mcu_color(const uint8_t* pix, long long pitch, int W, int H, int mx, int my, const Tables* t,
                      int16_t* coef /* 6 x 64 */, uint64_t* mask /* 6 */) {
	const int wb = (W + 7) >> 3, hb = (H + 7) >> 3;   // Y blocks that hold image samples
	int d[64];
	int16_t dc[4] = { 0, 0, 0, 0 };
	for (int b = 0; b < 4; ++b) {
		const int bx = 2 * mx + (b & 1), by = 2 * my + (b >> 1);
		int16_t* o = coef + 64 * b;
		if (by >= hb || bx >= wb) {   // jccoefct.c dummy blocks: zero, DC of the block before (bottom row: of Y01)
			for (int k = 0; k < 64; ++k) o[k] = 0;
			o[0] = by >= hb ? dc[1] : dc[b - 1];
			dc[b] = o[0];
			mask[b] = o[0] ? 1 : 0;
			continue;
		}
		for (int v = 0; v < 8; ++v) {
			const int y = imin(8 * by + v, H - 1);
			const uint8_t* row = pix + (long long)y * pitch;
			for (int u = 0; u < 8; ++u) {
				int Y, Cb, Cr;
				ycc(row + 3 * imin(8 * bx + u, W - 1), Y, Cb, Cr);
				d[8 * v + u] = Y - 128;
			}
		}
		mask[b] = fdct_quant(d, t, 0, o);
		dc[b] = o[0];
	}
	// chroma: rows past the last down-sampled row repeat it; columns past the image repeat the last input column
	const int ch = (H + 1) >> 1;
	for (int c = 0; c < 2; ++c) {
		for (int v = 0; v < 8; ++v) {
			const int j = imin(8 * my + v, ch - 1);
			const uint8_t* r0 = pix + (long long)imin(2 * j, H - 1) * pitch;
			const uint8_t* r1 = pix + (long long)imin(2 * j + 1, H - 1) * pitch;
			for (int u = 0; u < 8; ++u) {
				const int i = 8 * mx + u;
				const int x0 = 3 * imin(2 * i, W - 1), x1 = 3 * imin(2 * i + 1, W - 1);
				int s = 1 + (u & 1);   // jcsample.c h2v2_downsample: bias 1, 2, 1, 2, ...
				int Y, Cb, Cr;
				ycc(r0 + x0, Y, Cb, Cr); s += c ? Cr : Cb;
				ycc(r0 + x1, Y, Cb, Cr); s += c ? Cr : Cb;
				ycc(r1 + x0, Y, Cb, Cr); s += c ? Cr : Cb;
				ycc(r1 + x1, Y, Cb, Cr); s += c ? Cr : Cb;
				d[8 * v + u] = (s >> 2) - 128;
			}
		}
		mask[4 + c] = fdct_quant(d, t, 1, coef + 64 * (4 + c));
	}
}

// One block of a 1-channel image (non-interleaved scan: MCU = one block).
DVP_JHD void mcu_grey(const uint8_t* pix, long long pitch, int W, int H, int bx, int by, const Tables* t, int16_t* coef, uint64_t* mask) {
	int d[64];
	for (int v = 0; v < 8; ++v) {
		const uint8_t* row = pix + (long long)imin(8 * by + v, H - 1) * pitch;
		for (int u = 0; u < 8; ++u) d[8 * v + u] = (int)row[imin(8 * bx + u, W - 1)] - 128;
	}
	*mask = fdct_quant(d, t, 0, coef);
}

// Entropy coding of one restart segment (jchuff.c encode_one_block, flush_bits).  `Out` receives bytes; 0xFF is followed
// by a stuffed 0x00 and the last partial byte is filled with ones.
struct CountOut { unsigned long long n = 0; DVP_JHD void put(uint8_t) { ++n; } };
struct WriteOut { uint8_t* p; DVP_JHD void put(uint8_t b) { *p++ = b; } };

template <class Out>
struct BitWriter {
	Out& out;
	uint32_t acc = 0;
	int n = 0;
	DVP_JHD explicit BitWriter(Out& o) : out(o) {}
	DVP_JHD void emit(uint32_t code, int size) {
		acc = (acc << size) | (code & ((1u << size) - 1u));
		n += size;
		while (n >= 8) {
			n -= 8;
			const uint8_t b = (uint8_t)(acc >> n);
			out.put(b);
			if (b == 0xFF) out.put(0);
		}
		acc &= (1u << n) - 1u;
	}
	DVP_JHD void flush() {
		if (n) emit(0x7F, 8 - n);
	}
};

DVP_JHD int nbits(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

template <class Out>
DVP_JHD void code_segment(const Tables* t, const int16_t* coef, const uint64_t* mask, long long first_mcu, long long n_mcu, int bpm, Out& out) {
	BitWriter<Out> bw(out);
	int last_dc[3] = { 0, 0, 0 };
	for (long long m = first_mcu; m < first_mcu + n_mcu; ++m) {
		for (int b = 0; b < bpm; ++b) {
			const int comp = b < 4 ? 0 : b - 3, tbl = comp ? 1 : 0;
			const long long blk = m * bpm + b;
			const int16_t* c = coef + blk * 64;
			int v = c[0] - last_dc[comp];
			last_dc[comp] = c[0];
			int a = v < 0 ? -v : v, nb = nbits(a);
			uint32_t h = t->dc[tbl][nb];
			bw.emit(h & 0xFFFF, h >> 16);
			if (nb) bw.emit((uint32_t)(v < 0 ? v - 1 : v), nb);
			uint64_t mk = mask[blk] & ~(uint64_t)1;
			int last = 0;
			while (mk) {
				const int k = __builtin_ctzll(mk);
				mk &= mk - 1;
				int r = k - last - 1;
				while (r > 15) { h = t->ac[tbl][0xF0]; bw.emit(h & 0xFFFF, h >> 16); r -= 16; }
				v = c[k]; a = v < 0 ? -v : v; nb = nbits(a);
				h = t->ac[tbl][(r << 4) + nb];
				bw.emit(h & 0xFFFF, h >> 16);
				bw.emit((uint32_t)(v < 0 ? v - 1 : v), nb);
				last = k;
			}
			if (last != 63) { h = t->ac[tbl][0]; bw.emit(h & 0xFFFF, h >> 16); }
		}
	}
	bw.flush();
}

// ---- preview renderers (APD.cpp:694-812), BGR -------------------------------------------------------------------------
// The maps are what dvp_unpack_maps / the driver's unpack loop make of a plane: depth = plane.w inside [dmin, dmax], else 0
// (NaN kept); state = weak_info, or UNKNOWN where the depth is out of range.
DVP_JHD void render_depth(float d, float dmin, float dmax, uint8_t* o) {   // ShowDepthMap, APD.cpp:694-758
	o[0] = o[1] = o[2] = 0;
	if (d < dmin || d > dmax || d != d) return;
	float pv = (dmax - d) / (dmax - dmin);
	if (pv > 1) pv = 1;
	if (pv < 0) pv = 0;
	pv = pv * 255;
	if (pv > 255) pv = 255;
	else if (pv < 0) pv = 0;
	if (pv <= 51) { o[0] = 255; o[1] = (uint8_t)(pv * 5); o[2] = 0; }
	else if (pv <= 102) { pv -= 51; o[0] = (uint8_t)(255 - pv * 5); o[1] = 255; o[2] = 0; }
	else if (pv <= 153) { pv -= 102; o[0] = 0; o[1] = 255; o[2] = (uint8_t)(pv * 5); }
	else if (pv <= 204) { pv -= 153; o[0] = 0; o[1] = (uint8_t)(255 - (int)(uint8_t)((double)pv * 128.0 / 51 + 0.5)); o[2] = 255; }
	else if (pv <= 255) { pv -= 204; o[0] = 0; o[1] = (uint8_t)(127 - (int)(uint8_t)((double)pv * 127.0 / 51 + 0.5)); o[2] = 255; }
}

DVP_JHD uint8_t sat_u8(float v) {   // saturate_cast<uchar>(float): round half to even, NaN -> 0, clamp
	if (!(v == v)) return 0;
	const float r = rintf(v);
	return r <= 0.0f ? 0 : (r >= 255.0f ? 255 : (uint8_t)r);
}

DVP_JHD void render_normal(float x, float y, float z, uint8_t* o) {   // ShowNormalMap, APD.cpp:760-783
	const float norm = (float)sqrt((double)x * (double)x + (double)y * (double)y + (double)z * (double)z);
	float n[3] = { 0.0f, 0.0f, 0.0f };
	if (!(norm == 0)) {
		const float inv = 1.f / norm;
		n[0] = x * inv; n[1] = y * inv; n[2] = z * inv;
	}
	for (int i = 0; i < 3; ++i) {
		const float s = n[i] * 127.5f;   // convertTo(CV_8UC3, 127.5, 127.5), unfused
		o[i] = sat_u8(s + 127.5f);
	}
}

DVP_JHD void render_weak(uint8_t s, uint8_t* o) {   // ShowWeakImage, APD.cpp:785-812 (other values: black)
	o[0] = s == 0 ? 255 : 0;
	o[1] = s <= 1 ? 255 : 0;
	o[2] = (s == 0 || s == 2) ? 255 : 0;
}


// ---- host side: tables and the header segments --------------------------------------------------------------------------
// jpeg_set_quality (jcparam.c): Annex K tables scaled, clamped to [1, 255] (force_baseline)
inline void build_tables(int quality, Tables* t) {
	static const uint8_t natural[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
		7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
	static const uint8_t base[2][64] = {   // natural order
		{ 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
		  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 },
		{ 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
		  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 } };
	// the standard Huffman tables (Annex K.3): code lengths 1..16, then the symbols
	static const uint8_t dc_bits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
	static const uint8_t ac_bits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125 }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119 } };
	static const uint8_t ac_vals[2][162] = {
		{ 1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98,
		  114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86,
		  87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138,
		  146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
		  194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233,
		  234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250 },
		{ 0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
		  209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
		  86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136,
		  137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
		  185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232,
		  233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250 } };
	// jdhuff.c / jchuff.c jpeg_make_c_derived_tbl: canonical codes in order of length
	auto derive = [](const uint8_t* bits, const uint8_t* vals, uint32_t* out, int n_out) {
		for (int i = 0; i < n_out; ++i) out[i] = 0;
		uint32_t code = 0;
		int k = 0;
		for (int len = 1; len <= 16; ++len) {
			for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)len << 16) | code++;
			code <<= 1;
		}
	};
	static const uint8_t dc_vals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
	const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
	const int scale = q < 50 ? 5000 / q : 200 - q * 2;
	for (int c = 0; c < 2; ++c) {
		derive(dc_bits[c], dc_vals, t->dc[c], 12);
		derive(ac_bits[c], ac_vals[c], t->ac[c], 256);
		for (int k = 0; k < 64; ++k) {
			long v = ((long)base[c][natural[k]] * scale + 50L) / 100L;
			v = v < 1 ? 1 : (v > 255 ? 255 : v);
			t->qval[c][k] = (uint8_t)v;
			t->qdiv[c][k] = (uint16_t)(v << 3);
		}
	}
	for (int k = 0; k < 64; ++k) t->natural[k] = natural[k];
}

// SOI APP0(JFIF 1.01) DQT.. SOF0 DHT.. DRI SOS, in libjpeg's order (jcmarker.c); returns the byte count (<= 1024)
inline int build_header(const Tables* t, int W, int H, int C, int restart, uint8_t* o) {
	int n = 0;
	auto b = [&](int v) { o[n++] = (uint8_t)v; };
	auto w = [&](int v) { b(v >> 8); b(v & 0xFF); };
	w(0xFFD8);
	w(0xFFE0); w(16); b('J'); b('F'); b('I'); b('F'); b(0); b(1); b(1); b(0); w(1); w(1); b(0); b(0);
	const int ntab = C == 3 ? 2 : 1;
	for (int c = 0; c < ntab; ++c) { w(0xFFDB); w(67); b(c); for (int k = 0; k < 64; ++k) b(t->qval[c][k]); }
	w(0xFFC0); w(8 + 3 * C); b(8); w(H); w(W); b(C);
	for (int c = 0; c < C; ++c) { b(c + 1); b(c == 0 && C == 3 ? 0x22 : 0x11); b(c ? 1 : 0); }
	for (int c = 0; c < ntab; ++c) {
		for (int ac = 0; ac < 2; ++ac) {
			const uint32_t* tab = ac ? t->ac[c] : t->dc[c];
			const int nsym = ac ? 256 : 12;
			uint8_t bits[16] = { 0 };
			int cnt = 0;
			for (int s = 0; s < nsym; ++s) if (tab[s]) { ++bits[(tab[s] >> 16) - 1]; ++cnt; }
			w(0xFFC4); w(2 + 1 + 16 + cnt); b((ac << 4) | c);
			for (int i = 0; i < 16; ++i) b(bits[i]);
			uint32_t key[256];   // symbols in code order: (length, code) ascending
			int m = 0;
			for (int s = 0; s < nsym; ++s) {
				if (!tab[s]) continue;
				uint32_t e = ((tab[s] >> 16) << 24) | ((tab[s] & 0xFFFF) << 8) | (uint32_t)s;
				int i = m++;
				while (i > 0 && key[i - 1] > e) { key[i] = key[i - 1]; --i; }
				key[i] = e;
			}
			for (int i = 0; i < m; ++i) b(key[i] & 0xFF);
		}
	}
	w(0xFFDD); w(4); w(restart);
	w(0xFFDA); w(6 + 2 * C); b(C);
	for (int c = 0; c < C; ++c) { b(c + 1); b(c ? 0x11 : 0x00); }
	b(0); b(63); b(0);
	return n;
}

}   // namespace dvpjpeg
#endif
