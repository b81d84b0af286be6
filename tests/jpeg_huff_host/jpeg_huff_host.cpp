// jpeg_huff_host.cpp — the parallel Huffman scan of csrc/dvp_jpeg_huff.hpp emulated on the host (TEST INFRASTRUCTURE): the passes
// that the kernels of csrc/dvp_jpeg_huff.hip run a lane per subsequence are run here with serial loops over the lanes, in forward
// and in reverse lane order within a step, on arrays of exactly the sizes the device path allocates (the address sanitizer sees
// every index).  The offsets and records that come out are compared word for word with Decoder::scan's.
//   jpeg_huff_host check in.jpg subseq_bytes luma_only round_cap
//       exit 0: the emulation gave the serial scan's words in both orders, or left the file to the serial scan (then `path` says why)
//       exit 3: a difference, or the emulation accepted what the serial scan refuses
//       stdout: path device|host|fellback  why ...  segments N subsequences N chunks N longest N rounds N decodes N straddles N
//               serial ok|<the serial scan's message>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_jpeg_dec_mid.hpp"
#include "../../dvp-mvs_amd/csrc/dvp_jpeg_huff.hpp"

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

struct Outcome {
	bool device = false;
	const char* why = "";
	std::vector<uint32_t> offsets[3], records[3];
	uint32_t longest = 0, rounds = 0, decodes = 0;
};

template <class T, class S>
static void inclusive_scan(const T* in, size_t n, S* out) {
	S sum = 0;
	for (size_t k = 0; k < n; ++k) { sum += (S)in[k]; out[k] = sum; }
}

// the launches of csrc/dvp_jpeg_huff.hip, one after the other; `reverse`: the lanes of a step in descending order
static Outcome emulate(const dvpjh::Plan& pl, bool reverse, int round_cap, int subseq_bytes) {
	using namespace dvpjh;
	Outcome out;
	const uint32_t lanes = pl.lanes, chunks = pl.chunks;
	std::vector<uint8_t> bytes(pl.data, pl.data + pl.data_bytes);   // a copy of exactly the uploaded bytes
	std::vector<unsigned long long> st(lanes), carry0(chunks), carry1(chunks);
	std::vector<uint32_t> began(lanes), first_block(lanes + 1, 0), counters(kCounters, 0);
	std::vector<int32_t> dc[3];
	std::vector<long long> dc_sum[3];
	Job j;
	memset(&j, 0, sizeof(j));
	j.bytes = bytes.data(); j.segs = pl.segs.data(); j.lane_seg = pl.lane_seg.data(); j.tables = &pl.tables;
	j.lanes = lanes; j.segments = (uint32_t)pl.segs.size(); j.chunks = chunks; j.subseq_bytes = subseq_bytes;
	j.st = st.data(); j.carry[0] = carry0.data(); j.carry[1] = carry1.data(); j.began = began.data(); j.first_block = first_block.data();
	j.counters = counters.data();
	j.lay = pl.lay;
	for (int i = 0; i < pl.lay.comps; ++i) {
		dc[i].assign(pl.blocks[i], 0);
		dc_sum[i].assign(pl.blocks[i], 0);
		j.dc[i] = dc[i].data();
		j.dc_sum[i] = dc_sum[i].data();
		if (pl.lay.c[i].want) { out.offsets[i].assign(pl.blocks[i] + 1, 0); j.offsets[i] = out.offsets[i].data(); }
	}
	const Tables& T = pl.tables;
	auto each = [&](uint32_t n, auto&& f) {
		if (reverse) for (uint32_t k = n; k-- > 0;) f(k);
		else for (uint32_t k = 0; k < n; ++k) f(k);
	};
	each(lanes, [&](uint32_t l) { init_lane(j, l); });
	// the synchronisation inside the chunks
	bool changed = false;
	for (uint32_t c = 0; c < chunks; ++c) {
		const uint32_t first = c * kChunkLanes, n = std::min<uint32_t>(kChunkLanes, lanes - first);
		std::vector<uint32_t> at(n), steps(n, 0);
		std::vector<State> s(n);
		std::vector<char> active(n, 1);
		for (uint32_t k = 0; k < n; ++k) { at[k] = first + k; s[k] = unpack(st[first + k]); }
		for (int t = 0; t < kChunkLanes; ++t) {
			bool any = false;
			each(n, [&](uint32_t k) {
				if (!active[k]) return;
				bool carried = false;
				active[k] = sync_step(j, T, &at[k], &s[k], &carried);
				++steps[k];
				changed |= carried;
				any |= active[k] != 0;
			});
			if (!any) break;
		}
		for (uint32_t k = 0; k < n; ++k) { out.longest = std::max(out.longest, steps[k]); out.decodes += steps[k]; }
	}
	// the rounds across the chunks
	int from = 0;
	while (changed) {
		if ((int)out.rounds >= round_cap) { out.why = "round cap"; return out; }
		changed = false;
		each(chunks, [&](uint32_t c) {
			bool carried = false;
			const uint32_t d = round_chunk(j, T, c, from, &carried);
			out.decodes += d;
			out.longest = std::max(out.longest, d);
			changed |= carried;
		});
		from = 1 - from;
		++out.rounds;
	}
	bool flag = false;
	each(lanes, [&](uint32_t l) { if (!census_lane(j, T, l)) flag = true; });
	inclusive_scan(began.data(), lanes, first_block.data() + 1);
	each(lanes, [&](uint32_t l) { if (!count_lane(j, T, l)) flag = true; });
	for (int i = 0; i < pl.lay.comps; ++i) {
		if (j.offsets[i]) inclusive_scan(j.offsets[i] + 1, pl.blocks[i], j.offsets[i] + 1);
		inclusive_scan(j.dc[i], pl.blocks[i], j.dc_sum[i]);
		each((uint32_t)pl.blocks[i], [&](uint32_t b) { if (!finish_dc(j, i, b)) flag = true; });
	}
	if (flag) { out.why = "flag"; return out; }
	for (int i = 0; i < pl.lay.comps; ++i)
		if (j.offsets[i]) { out.records[i].assign(out.offsets[i][pl.blocks[i]], 0xDEADBEEFu); j.records[i] = out.records[i].data(); }
	each(lanes, [&](uint32_t l) { write_lane(j, T, l); });
	out.device = true;
	return out;
}

// 0xFF 0x00 pairs whose two bytes lie in different subsequences
static long long straddles(const dvpjh::Plan& pl, int subseq_bytes) {
	long long n = 0;
	for (const dvpjh::Seg& sg : pl.segs)
		for (uint32_t o = (uint32_t)subseq_bytes; o < sg.len; o += (uint32_t)subseq_bytes)
			n += pl.data[sg.start + o] == 0 && pl.data[sg.start + o - 1] == 0xFF;
	return n;
}

static std::string word(const char* text) {   // one word: the line is parsed by splitting at blanks
	std::string w(text);
	for (char& c : w) if (c == ' ') c = '_';
	return w.empty() ? "-" : w;
}

static int check(const char* in, int subseq_bytes, bool luma_only, int round_cap) {
	std::vector<uint8_t> file;
	if (!read_file(in, &file)) { fprintf(stderr, "cannot read %s\n", in); return 1; }
	Decoder serial;
	const bool serial_ok = serial.decode(file.data(), file.size(), luma_only);
	Decoder d;
	d.stop_at_scan = true;
	dvpjh::Plan pl;
	const bool parsed = d.decode(file.data(), file.size(), luma_only);
	const bool planned = parsed && dvpjh::plan(d, luma_only, subseq_bytes, &pl);
	int rc = 0;
	if (!planned) {
		printf("path host why %s segments 0 subsequences 0 chunks 0 longest 0 rounds 0 decodes 0 straddles 0", word(parsed ? pl.why_not : d.error).c_str());
	} else {
		Outcome o[2] = { emulate(pl, false, round_cap, subseq_bytes), emulate(pl, true, round_cap, subseq_bytes) };
		if (o[0].device != o[1].device || o[0].rounds != o[1].rounds || o[0].longest != o[1].longest || o[0].decodes != o[1].decodes) { fprintf(stderr, "the two lane orders ran differently\n"); rc = 3; }
		for (const Outcome& e : o) {
			if (!e.device) continue;
			if (!serial_ok) { fprintf(stderr, "accepted a file the serial scan refuses (%s)\n", serial.error); rc = 3; continue; }
			for (size_t i = 0; i < serial.comps.size(); ++i)
				if (e.offsets[i] != serial.comps[i].offsets || e.records[i] != serial.comps[i].records) { fprintf(stderr, "component %zu differs from the serial scan\n", i); rc = 3; }
		}
		printf("path %s why %s segments %zu subsequences %u chunks %u longest %u rounds %u decodes %u straddles %lld", o[0].device ? "device" : "fellback", word(o[0].why).c_str(),
		       pl.segs.size(), pl.lanes, pl.chunks, o[0].longest, o[0].rounds, o[0].decodes, straddles(pl, subseq_bytes));
	}
	printf(" serial %s\n", serial_ok ? "ok" : word(serial.error).c_str());
	return rc;
}

int main(int argc, char** argv) {
	if (argc == 6 && std::string(argv[1]) == "check") return check(argv[2], atoi(argv[3]), atoi(argv[4]) != 0, atoi(argv[5]));
	printf("usage: jpeg_huff_host check in.jpg subseq_bytes luma_only round_cap\n");
	return 64;
}
