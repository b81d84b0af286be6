// jpeg_dec_host.cpp — the input JPEG decoder's shared text built for the host (TEST INFRASTRUCTURE): csrc/dvp_jpeg_dec_mid.hpp
// (parse + entropy decode -> coefficient records) and csrc/dvp_jpeg_dec.hpp (block and pixel arithmetic), run block after block and
// pixel after pixel, without the host mirror's Mat and without HIP.  tests/test_jpeg_dec_host.py compares its output with the
// host mirror's DecodeJpeg and with libjpeg.
//   jpeg_dec_host decode in.jpg out.bin channels   int32 rows, cols, channels + the bytes; a rejected file: exit 2, the message
//                                                  on stderr, out.bin not written
//   jpeg_dec_host records in.jpg out.bin           per component the int32 coefficients [block][64] that the records give
//                                                  (densified, dequantised), preceded by int32 components and, per component,
//                                                  int32 blocks_w, blocks_h; exit 3 if they differ from a dense decode of the
//                                                  same scan (below); statistics of the records on stdout
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_jpeg_dec.hpp"
#include "../../dvp-mvs_amd/csrc/dvp_jpeg_dec_mid.hpp"

using dvpjdmid::Component;
using dvpjdmid::Decoder;

static bool read_file(const char* name, std::vector<uint8_t>* out) {
	FILE* f = fopen(name, "rb");
	if (!f) return false;
	uint8_t buf[65536];
	size_t n;
	while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + n);
	fclose(f);
	return true;
}

static bool write_file(const char* name, const std::vector<uint8_t>& header, const std::vector<uint8_t>& body) {
	FILE* f = fopen(name, "wb");
	if (!f) return false;
	const bool ok = fwrite(header.data(), 1, header.size(), f) == header.size() && fwrite(body.data(), 1, body.size(), f) == body.size();
	fclose(f);
	return ok;
}

static void put_i32(std::vector<uint8_t>* v, int32_t x) { const uint8_t* p = (const uint8_t*)&x; v->insert(v->end(), p, p + 4); }

static std::vector<uint8_t> plane_of(const Decoder& d, const Component& c) {
	const size_t pitch = (size_t)c.blocks_w * 8;
	std::vector<uint8_t> plane(pitch * c.blocks_h * 8);
	const size_t blocks = (size_t)c.blocks_w * c.blocks_h;
	for (size_t b = 0; b < blocks; ++b)
		dvpjd::reconstruct_block(c.records.data() + c.offsets[b], c.offsets[b + 1] - c.offsets[b], d.qt[c.tq], plane.data() + (b / c.blocks_w) * 8 * pitch + (b % c.blocks_w) * 8, pitch);
	return plane;
}

static int decode(const char* in, const char* out, int channels) {
	std::vector<uint8_t> file;
	if (!read_file(in, &file)) { fprintf(stderr, "cannot read %s\n", in); return 1; }
	Decoder d;
	if (!d.decode(file.data(), file.size(), channels == 1)) { fprintf(stderr, "jpeg_dec_host: %s: %s\n", in, d.error); return 2; }
	std::vector<uint8_t> header, body((size_t)d.width * d.height * channels);
	put_i32(&header, d.height); put_i32(&header, d.width); put_i32(&header, channels);
	const int n = channels == 1 ? 1 : (int)d.comps.size();
	std::vector<uint8_t> planes[3];
	for (int i = 0; i < n; ++i) planes[i] = plane_of(d, d.comps[i]);
	auto sample = [&](int i, int x, int y) {
		const Component& c = d.comps[i];
		return (int)planes[i][(size_t)dvpjd::sample_row(y, c.v, d.vmax) * c.blocks_w * 8 + (size_t)dvpjd::sample_col(x, c.h, d.hmax)];
	};
	for (int y = 0; y < d.height; ++y)
		for (int x = 0; x < d.width; ++x) {
			uint8_t* o = body.data() + ((size_t)y * d.width + x) * channels;
			const int yy = sample(0, x, y);
			if (channels == 1) o[0] = (uint8_t)yy;
			else if (n == 3) dvpjd::ycc_to_bgr(yy, sample(1, x, y), sample(2, x, y), o);
			else o[0] = o[1] = o[2] = (uint8_t)yy;
		}
	return write_file(out, header, body) ? 0 : 1;
}

// The scan decoded densely, the way a decoder without records does it: 64 dequantised coefficients per block, written where the
// block lies.  Uses the tables the parse left in `d` and walks the scan again from the SOS segment.
static bool dense_scan(const Decoder& d, const std::vector<uint8_t>& file, std::vector<std::vector<int32_t>>* coef) {
	size_t p = 2;
	const uint8_t* data = nullptr;
	while (p + 4 <= file.size()) {
		if (file[p] != 0xFF) { ++p; continue; }
		const int marker = file[p + 1];
		p += 2;
		if (marker == 0xD8 || (marker >= 0xD0 && marker <= 0xD7) || marker == 0x01) continue;
		if (marker == 0xFF) { --p; continue; }
		const size_t len = ((size_t)file[p] << 8) | file[p + 1];
		if (marker == 0xDA) { data = file.data() + p + len; break; }
		p += len;
	}
	if (!data) return false;
	const uint8_t* zz = dvpjdmid::zigzag();
	coef->assign(d.comps.size(), std::vector<int32_t>());
	std::vector<int> pred(d.comps.size(), 0);
	for (size_t i = 0; i < d.comps.size(); ++i) (*coef)[i].assign((size_t)d.comps[i].blocks_w * d.comps[i].blocks_h * 64, 0);
	dvpjdmid::BitReader br{ data, file.data() + file.size() };
	const int mcus_x = d.comps[0].blocks_w / d.comps[0].h, mcus_y = d.comps[0].blocks_h / d.comps[0].v;
	int until = d.restart_interval;
	for (int my = 0; my < mcus_y; ++my)
		for (int mx = 0; mx < mcus_x; ++mx) {
			if (d.restart_interval && until == 0) {
				const uint8_t* q = br.p;
				while (q + 1 < br.end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) ++q;
				if (q + 1 >= br.end) return false;
				br.p = q + 2;
				br.reset();
				for (int& v : pred) v = 0;
				until = d.restart_interval;
			}
			for (size_t i = 0; i < d.comps.size(); ++i) {
				const Component& c = d.comps[i];
				for (int by = 0; by < c.v; ++by)
					for (int bx = 0; bx < c.h; ++bx) {
						int32_t* out = (*coef)[i].data() + ((size_t)(my * c.v + by) * c.blocks_w + (size_t)(mx * c.h + bx)) * 64;
						const int t = dvpjdmid::decode_symbol(br, d.dc[c.td]);
						if (t < 0 || t > 11) return false;
						if (t) pred[i] += dvpjdmid::extend(br.get(t), t);
						out[0] = pred[i] * d.qt[c.tq][0];
						for (int k = 1; k < 64;) {
							const int rs = dvpjdmid::decode_symbol(br, d.ac[c.ta]);
							if (rs < 0) return false;
							const int r = rs >> 4, sz = rs & 15;
							if (sz == 0) { if (r == 15) { k += 16; continue; } break; }
							k += r;
							if (k > 63) return false;
							out[zz[k]] = dvpjdmid::extend(br.get(sz), sz) * d.qt[c.tq][zz[k]];
							++k;
						}
					}
			}
			if (d.restart_interval) --until;
		}
	return true;
}

static int records(const char* in, const char* out) {
	std::vector<uint8_t> file;
	if (!read_file(in, &file)) { fprintf(stderr, "cannot read %s\n", in); return 1; }
	Decoder d;
	if (!d.decode(file.data(), file.size(), false)) { fprintf(stderr, "jpeg_dec_host: %s: %s\n", in, d.error); return 2; }
	std::vector<std::vector<int32_t>> dense;
	if (!dense_scan(d, file, &dense)) { fprintf(stderr, "jpeg_dec_host: the dense decode of %s failed\n", in); return 3; }
	std::vector<uint8_t> header, body;
	put_i32(&header, (int32_t)d.comps.size());
	long long blocks = 0, min_records = 64, max_records = 0, zero_dc = 0, clamp_low = 0, clamp_high = 0, record_bytes = 0, differ = 0;
	for (size_t i = 0; i < d.comps.size(); ++i) {
		const Component& c = d.comps[i];
		put_i32(&header, c.blocks_w); put_i32(&header, c.blocks_h);
		const size_t n = (size_t)c.blocks_w * c.blocks_h;
		record_bytes += (long long)(c.offsets.size() + c.records.size()) * 4;
		for (size_t b = 0; b < n; ++b) {
			const uint32_t* r = c.records.data() + c.offsets[b];
			const long long count = c.offsets[b + 1] - c.offsets[b];
			int coef[64];
			dvpjd::densify(r, (uint32_t)count, d.qt[c.tq], coef);
			differ += memcmp(coef, dense[i].data() + b * 64, sizeof(coef)) != 0;
			const uint8_t* bytes = (const uint8_t*)coef;
			body.insert(body.end(), bytes, bytes + sizeof(coef));
			++blocks;
			min_records = count < min_records ? count : min_records;
			max_records = count > max_records ? count : max_records;
			zero_dc += count >= 1 && dvpjd::record_position(r[0]) == 0 && dvpjd::record_value(r[0]) == 0;
			// the samples before the clamp
			int ws[64];
			memcpy(ws, coef, sizeof(ws));
			for (int col = 0; col < 8; ++col) dvpjd::idct_column(ws, ws, 8, col);
			for (int row = 0; row < 8; ++row) {
				long long o[8];
				const int* p = ws + 8 * row;
				dvpjd::idct_line(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], o);
				for (int col = 0; col < 8; ++col) {
					const int v = dvpjd::descale(o[col], dvpjd::CONST_BITS + dvpjd::PASS1_BITS + 3) + 128;
					clamp_low += v < 0;
					clamp_high += v > 255;
				}
			}
		}
	}
	printf("blocks %lld min_records %lld max_records %lld zero_dc %lld clamp_low %lld clamp_high %lld record_bytes %lld differ %lld\n", blocks, min_records, max_records, zero_dc, clamp_low,
	       clamp_high, record_bytes, differ);
	if (differ) return 3;
	return write_file(out, header, body) ? 0 : 1;
}

int main(int argc, char** argv) {
	if (argc == 5 && std::string(argv[1]) == "decode" && (std::string(argv[4]) == "1" || std::string(argv[4]) == "3")) return decode(argv[2], argv[3], atoi(argv[4]));
	if (argc == 4 && std::string(argv[1]) == "records") return records(argv[2], argv[3]);
	printf("usage: jpeg_dec_host decode in.jpg out.bin 1|3 | records in.jpg out.bin\n");
	return 64;
}
