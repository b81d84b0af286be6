// dvp_jpeg_dec_mid.hpp — the sequential half of the input JPEG decoder: marker parse, tables and the Huffman entropy decode of a
// baseline / extended-sequential 8-bit file (DQT, DHT, SOF0 / SOF1, DRI, SOS, restart markers).  Plain C++ on plain arrays: the host
// mirror (host/jpeg.cpp) and the engine library (csrc/dvp_jpeg_dec.hip) include this one text, so a file is accepted or rejected —
// with one message — the same way wherever it is decoded.  What is independent per block (dequantisation, inverse DCT, clamp) and
// per pixel (chroma sampling, colour equations) is in dvp_jpeg_dec.hpp.
//
// The scan is not expanded into dense blocks of 64 coefficients; it leaves COEFFICIENT RECORDS per component:
//   offsets[b]   uint32, b = 0 ... blocks_w * blocks_h, in the component's block raster order (the component padded to whole MCUs):
//                the records of block b are records[offsets[b] ... offsets[b + 1])
//   records[k]   uint32, one per non-zero QUANTISED coefficient: natural-order position (0 ... 63) in the low 6 bits, the signed
//                value above them (an AC value fits 16 bits; the field is sign-extended over all 26 so that a DC prediction
//                that has run out of 16 bits in a damaged file is still kept as the dense decoder kept it).  In the order of the
//                scan, i.e. in zig-zag order of the positions.
// The first record of a block is its DC value — the running prediction — and is written even when it is zero: every block has
// at least one record, and a flat block has exactly one.  With luma_only the chroma blocks are entropy-decoded, as the stream
// demands, but leave no records.  Quantisation tables are 4 x 64 uint16 in natural order.
#ifndef DVP_JPEG_DEC_MID_HPP_
#define DVP_JPEG_DEC_MID_HPP_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dvpjdmid {

struct Huff {
	uint8_t bits[17] = { 0 };
	uint8_t vals[256] = { 0 };
	int mincode[17], maxcode[18], valptr[17];
	bool ok = false;
	void build() {
		int code = 0, k = 0;
		for (int l = 1; l <= 16; ++l) {
			valptr[l] = k;
			mincode[l] = code;
			code += bits[l];
			k += bits[l];
			maxcode[l] = bits[l] ? code - 1 : -1;
			code <<= 1;
		}
		maxcode[17] = 0x7fffffff;
		ok = true;
	}
};

struct Component {
	int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
	int blocks_w = 0, blocks_h = 0;   // in 8x8 blocks, padded to whole MCUs
	int pred = 0;
	bool want = false;                // records are kept for this component
	std::vector<uint32_t> offsets;    // blocks_w * blocks_h + 1
	std::vector<uint32_t> records;
};

struct BitReader {
	const uint8_t* p;
	const uint8_t* end;
	uint32_t acc = 0;
	int nbits = 0;
	bool hit_marker = false;
	void fill() {
		while (nbits <= 24) {
			int byte = 0;
			if (!hit_marker && p < end) {
				byte = *p++;
				if (byte == 0xFF) {
					const int nxt = p < end ? *p : 0xD9;
					if (nxt == 0) ++p;                            // stuffed zero
					else { hit_marker = true; --p; byte = 0; }    // a marker: feed zeros from here on
				}
			}
			acc |= (uint32_t)byte << (24 - nbits);
			nbits += 8;
		}
	}
	int bit() { if (nbits < 1) fill(); const int b = acc >> 31; acc <<= 1; --nbits; return b; }
	int get(int n) {   // n <= 16
		if (n == 0) return 0;
		if (nbits < n) fill();
		const int v = (int)(acc >> (32 - n));
		acc <<= n;
		nbits -= n;
		return v;
	}
	void reset() { acc = 0; nbits = 0; hit_marker = false; }
};

inline int decode_symbol(BitReader& br, const Huff& h) {
	int code = 0;
	for (int l = 1; l <= 16; ++l) {
		code = (code << 1) | br.bit();
		if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) return h.vals[h.valptr[l] + code - h.mincode[l]];
	}
	return -1;
}
inline int extend(int v, int n) { return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v; }

inline const uint8_t* zigzag() {
	static const uint8_t k[64] = { 0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
		35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
	return k;
}

constexpr int kValueLimit = 1 << 25;   // |value| of a record stays below this: 26 bits above the position
inline uint32_t make_record(int position, int value) { return ((uint32_t)value << 6) | (uint32_t)position; }

// What a file says before its scan, and after decode() the records of the scan.  `file` must stay alive while decode() runs.
struct Decoder {
	uint16_t qt[4][64] = { { 0 } };
	bool have_qt[4] = { false, false, false, false };
	Huff dc[4], ac[4];
	std::vector<Component> comps;
	int width = 0, height = 0, hmax = 1, vmax = 1, restart_interval = 0;
	const char* error = "";
	// stop_at_scan: decode() reads everything up to the scan — tables, frame, DRI, the scan header — and returns true with
	// [scan_data, scan_end) the bytes behind the SOS segment, without running scan() (dvp_jpeg_huff.hpp decodes them in parallel)
	bool stop_at_scan = false;
	const uint8_t* scan_data = nullptr;
	const uint8_t* scan_end = nullptr;

	bool fail(const char* msg) { error = msg; return false; }
	int padded_width(const Component& c) const { return c.blocks_w * 8; }

	// header_only: stops at the frame header, with width, height and the components' sampling factors (no tables are needed)
	bool decode(const uint8_t* file, size_t file_bytes, bool luma_only, bool header_only = false) {
		const uint8_t* kZigzag = zigzag();
		const uint8_t* p = file;
		const uint8_t* end = p + file_bytes;
		if (file_bytes < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail("not a JPEG file");
		p += 2;
		while (p + 4 <= end) {
			if (*p != 0xFF) { ++p; continue; }
			const int marker = p[1];
			p += 2;
			if (marker == 0xD8 || (marker >= 0xD0 && marker <= 0xD7) || marker == 0x01 || marker == 0xFF) { if (marker == 0xFF) --p; continue; }
			if (marker == 0xD9) break;
			const int len = (p[0] << 8) | p[1];
			if (len < 2 || p + len > end) return fail("truncated segment");
			const uint8_t* s = p + 2;
			const uint8_t* se = p + len;
			if (marker == 0xDB) {
				while (s < se) {
					const int pq = *s >> 4, tq = *s & 15;
					++s;
					if (tq > 3) return fail("bad quantisation table id");
					if (s + (pq ? 128 : 64) > se) return fail("truncated segment");
					for (int i = 0; i < 64; ++i) {
						qt[tq][kZigzag[i]] = pq ? (uint16_t)((s[0] << 8) | s[1]) : *s;
						s += pq ? 2 : 1;
					}
					have_qt[tq] = true;
				}
			} else if (marker == 0xC4) {
				while (s < se) {
					const int tc = *s >> 4, th = *s & 15;
					++s;
					if (th > 3 || tc > 1) return fail("bad Huffman table id");
					Huff& h = tc ? ac[th] : dc[th];
					if (s + 16 > se) return fail("bad Huffman table");
					int total = 0;
					for (int l = 1; l <= 16; ++l) { h.bits[l] = *s++; total += h.bits[l]; }
					if (total > 256 || s + total > se) return fail("bad Huffman table");
					for (int i = 0; i < total; ++i) h.vals[i] = *s++;
					h.build();
				}
			} else if (marker == 0xC0 || marker == 0xC1) {
				if (len < 8) return fail("truncated segment");
				if (s[0] != 8) return fail("only 8-bit samples are supported");
				height = (s[1] << 8) | s[2];
				width = (s[3] << 8) | s[4];
				const int n = s[5];
				if (width <= 0 || height <= 0 || (n != 1 && n != 3)) return fail("unsupported frame (size / component count)");
				if (len < 8 + 3 * n) return fail("truncated segment");
				comps.assign(n, Component());
				hmax = vmax = 1;
				for (int i = 0; i < n; ++i) {
					comps[i].id = s[6 + 3 * i];
					comps[i].h = s[7 + 3 * i] >> 4;
					comps[i].v = s[7 + 3 * i] & 15;
					comps[i].tq = s[8 + 3 * i];
					if (comps[i].h < 1 || comps[i].h > 4 || comps[i].v < 1 || comps[i].v > 4 || comps[i].tq > 3) return fail("bad sampling factors");
					if (n == 1) comps[i].h = comps[i].v = 1;   // a single-component scan is never interleaved: one block per MCU
					hmax = std::max(hmax, comps[i].h);
					vmax = std::max(vmax, comps[i].v);
				}
				if (header_only) return true;
			} else if (marker == 0xC2 || (marker >= 0xC3 && marker <= 0xCF && marker != 0xC4 && marker != 0xC8 && marker != 0xCC)) {
				return fail("progressive / lossless / arithmetic-coded JPEG is not supported (baseline only)");
			} else if (marker == 0xDD) {
				if (len < 4) return fail("truncated segment");
				restart_interval = (s[0] << 8) | s[1];
			} else if (marker == 0xDA) {
				if (comps.empty()) return fail("scan before frame header");
				const int ns = s < se ? s[0] : 0;
				if (ns != (int)comps.size()) return fail("non-interleaved multi-scan files are not supported");
				if (len < 3 + 2 * ns) return fail("truncated segment");
				for (int i = 0; i < ns; ++i) {
					const int cid = s[1 + 2 * i];
					for (auto& c : comps)
						if (c.id == cid) { c.td = s[2 + 2 * i] >> 4; c.ta = s[2 + 2 * i] & 15; }
				}
				if (stop_at_scan) { scan_data = se; scan_end = end; return true; }
				if (!scan(se, end, luma_only)) return false;
				// a luma plane at reduced sampling would need interpolation; every encoder in practice gives luma full resolution
				if (luma_only && (comps[0].h != hmax || comps[0].v != vmax)) return fail("sub-sampled luma is not supported");
				return true;
			}
			p += len;
		}
		return fail(header_only ? "no frame header found" : "no scan found");
	}

	bool scan(const uint8_t* data, const uint8_t* end, bool luma_only) {
		const uint8_t* kZigzag = zigzag();
		const int mcu_w = 8 * hmax, mcu_h = 8 * vmax;
		const int mcus_x = (width + mcu_w - 1) / mcu_w, mcus_y = (height + mcu_h - 1) / mcu_h;
		for (auto& c : comps) {
			if (c.td > 3 || c.ta > 3) return fail("bad Huffman table id");
			if (!have_qt[c.tq] || !dc[c.td].ok || !ac[c.ta].ok) return fail("missing table");
			c.blocks_w = mcus_x * c.h;
			c.blocks_h = mcus_y * c.v;
			c.pred = 0;
			c.want = !luma_only || &c == &comps[0];
			c.records.clear();
			c.offsets.clear();
			if (c.want) {
				const size_t blocks = (size_t)c.blocks_w * c.blocks_h;
				c.offsets.assign(blocks + 1, 0);
				c.records.reserve(blocks * 6);   // (a photograph at the usual qualities: 4 ... 8 records per block)
			}
		}
		BitReader br{ data, end };
		int until_restart = restart_interval;
		for (int my = 0; my < mcus_y; ++my)
			for (int mx = 0; mx < mcus_x; ++mx) {
				if (restart_interval && until_restart == 0) {
					// byte-align, skip to the RSTn marker
					const uint8_t* q = br.p;
					while (q + 1 < end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) ++q;
					if (q + 1 >= end) return fail("missing restart marker");
					br.p = q + 2;
					br.reset();
					for (auto& c : comps) c.pred = 0;
					until_restart = restart_interval;
				}
				for (auto& c : comps) {
					const Huff& hd = dc[c.td];
					const Huff& ha = ac[c.ta];
					for (int by = 0; by < c.v; ++by)
						for (int bx = 0; bx < c.h; ++bx) {
							const int t = decode_symbol(br, hd);
							if (t < 0 || t > 11) return fail("corrupt DC code");
							if (t) c.pred += extend(br.get(t), t);
							if (c.pred <= -kValueLimit || c.pred >= kValueLimit) return fail("corrupt DC value");
							// the blocks of a component arrive MCU by MCU, not in raster order: the counts first, the offsets at the end
							const size_t block = (size_t)(my * c.v + by) * c.blocks_w + (size_t)(mx * c.h + bx);
							const size_t first = c.records.size();
							if (c.want) c.records.push_back(make_record(0, c.pred));
							for (int k = 1; k < 64;) {
								const int rs = decode_symbol(br, ha);
								if (rs < 0) return fail("corrupt AC code");
								const int r = rs >> 4, sz = rs & 15;
								if (sz == 0) { if (r == 15) { k += 16; continue; } break; }
								k += r;
								if (k > 63) return fail("corrupt AC run");
								const int value = extend(br.get(sz), sz);
								if (c.want && value != 0) c.records.push_back(make_record(kZigzag[k], value));
								++k;
							}
							if (c.want) c.offsets[block + 1] = (uint32_t)(c.records.size() - first);
						}
				}
				if (restart_interval) --until_restart;
			}
		for (auto& c : comps)
			if (c.want) raster_order(c);
		return true;
	}

private:
	// records were appended in scan order and offsets[b + 1] holds block b's count: when the component has more than one block per
	// MCU the scan order is not the raster order, and the records are regrouped.  (One block per MCU: the prefix sum is all.)
	void raster_order(Component& c) {
		const size_t blocks = (size_t)c.blocks_w * c.blocks_h;
		const bool in_order = c.h == 1 && c.v == 1;
		std::vector<uint32_t> count;
		if (!in_order) count.assign(c.offsets.begin() + 1, c.offsets.end());
		for (size_t b = 0; b < blocks; ++b) c.offsets[b + 1] += c.offsets[b];
		if (in_order) return;
		std::vector<uint32_t> sorted(c.records.size());
		const int mcus_x = c.blocks_w / c.h;
		size_t from = 0;
		const int mcus_y = c.blocks_h / c.v;
		for (int my = 0; my < mcus_y; ++my)
			for (int mx = 0; mx < mcus_x; ++mx)
				for (int by = 0; by < c.v; ++by)
					for (int bx = 0; bx < c.h; ++bx) {
						const size_t block = (size_t)(my * c.v + by) * c.blocks_w + (size_t)(mx * c.h + bx);
						std::copy(c.records.begin() + from, c.records.begin() + from + count[block], sorted.begin() + c.offsets[block]);
						from += count[block];
					}
		c.records.swap(sorted);
	}
};

}   // namespace dvpjdmid
#endif
