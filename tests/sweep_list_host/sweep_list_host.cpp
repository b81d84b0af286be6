// TEST INFRASTRUCTURE — the list-building functions of the sweep passes' evaluation launches (csrc/dvp_sweep_list.hpp) as a
// stand-alone host program under the address and undefined-behaviour sanitizers; run by tests/test_sweep_list_host.py.
//   sweep_list_host <case file> <result file>
// case file: int32 W, H, S, stage; then per pixel int32 flags (SWF_*), uint32 selected views, 32 weight bytes.
// result file: int32 R (kSweepListRounds), S, the S list lengths, then the S lists one after the other.
// The program itself checks what needs no second opinion: count + scan agree with the fill, nothing is written outside a list's
// entries, and for R = 2, 4, 8, 16 the workgroups of sweep_list_grid take every entry exactly once (sweep_list_chunk), in whole rounds
// except the list's last.
#include "../../dvp-mvs_amd/csrc/dvp_stages.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace dvp;

namespace {
long long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

template <class T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return fread(v.data(), sizeof(T), n, f) == n; }

int check_chunks(int n, int cap) {
	for (int rounds : { 2, 4, 8, 16 }) {
		const int grid = sweep_list_grid(cap, rounds);
		CHECK((long long)grid * 64 * rounds >= cap && (long long)(grid - 1) * 64 * rounds < cap);
		std::vector<int> hit((size_t)n, 0);
		int last = -1;
		for (int b = 0; b < grid; ++b) {
			const int c = sweep_list_chunk(b, n, rounds);
			if (c < 0) continue;
			CHECK(c == last + 1);   // chunk after chunk, each once
			last = c;
			const int first = c * 64 * rounds, end = first + 64 * rounds < n ? first + 64 * rounds : n;
			CHECK(first < n);
			CHECK(end == n || (end - first) % 64 == 0);   // only the list's last round is part-empty
			for (int i = first; i < end; ++i) hit[i]++;
		}
		for (int i = 0; i < n; ++i) CHECK(hit[i] == 1);
	}
	return 0;
}
}  // namespace

int main(int argc, char** argv) {
	if (argc != 3) { printf("usage: sweep_list_host <case file> <result file>\n"); return 2; }
	FILE* f = fopen(argv[1], "rb");
	if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
	int hdr[4];
	if (fread(hdr, 4, 4, f) != 4) { printf("short case file\n"); return 2; }
	const int W = hdr[0], H = hdr[1], S = hdr[2], stage = hdr[3];
	if (W < 1 || H < 1 || W >= 32768 || H >= 32768 || S < 1 || S > 32 || stage < 0 || stage > 1) { printf("bad case\n"); return 2; }
	const size_t L = (size_t)W * H;
	std::vector<int> flags;
	std::vector<uint32_t> sel;
	std::vector<uint8_t> vw;
	if (!read_n(f, flags, L) || !read_n(f, sel, L) || !read_n(f, vw, L * 32)) { printf("short case file\n"); return 2; }
	fclose(f);
	std::vector<f4> rec(2 * L, mk4(0, 0, 0, 0));
	for (size_t i = 0; i < L; ++i) rec[L + i].w = (float)flags[i];
	Dev d;
	std::memset(&d, 0, sizeof(d));
	d.width = W; d.height = H; d.num_images = S + 1; d.params.num_images = S + 1;
	d.sweep_rec = rec.data(); d.selected_views = sel.data(); d.view_weight = vw.data();
	const int cap = (int)L;
	const int tiles_x = (W + 63) / 64, tiles = tiles_x * ((H + kSweepRows - 1) / kSweepRows);
	const uint32_t kFill = 0xFFFFFFFFu;
	std::vector<int> counts((size_t)S * tiles, -1), n(S, -1);
	std::vector<uint32_t> list((size_t)S * cap, kFill);
	sweep_list_counts_host(d, tiles_x, tiles, 0, stage, counts.data());
	std::vector<int> per_tile = counts;
	sweep_list_scan_host(S, tiles, counts.data(), n.data());
	sweep_list_fill_host(d, tiles_x, tiles, 0, stage, counts.data(), list.data(), cap);
	for (int v = 0; v < S; ++v) {
		CHECK(n[v] >= 0 && n[v] <= cap);
		for (int t = 0; t < tiles; ++t) CHECK(counts[(size_t)v * tiles + t] + per_tile[(size_t)v * tiles + t] == (t + 1 < tiles ? counts[(size_t)v * tiles + t + 1] : n[v]));
		for (int i = 0; i < cap; ++i) {
			const uint32_t e = list[(size_t)v * cap + i];
			CHECK((e != kFill) == (i < n[v]));
			if (i < n[v]) {
				const int x = sweep_list_x(e), y = sweep_list_y(e);
				CHECK(x < W && y < H && sweep_list_pack(x, y) == e);
				CHECK(sweep_go(d, x + y * W, v, stage) && ((sweep_go_mask(d, x + y * W, stage) >> v) & 1u));
			}
		}
		if (check_chunks(n[v], cap)) return 1;
	}
	for (size_t c = 0; c < L; ++c)
		for (int v = 0; v < 32; ++v) CHECK(((sweep_go_mask(d, (int)c, stage) >> v) & 1u) == (v < S && sweep_go(d, (int)c, v, stage) ? 1u : 0u));
	FILE* o = fopen(argv[2], "wb");
	if (!o) { printf("cannot write %s\n", argv[2]); return 2; }
	const int head[2] = { kSweepListRounds, S };
	fwrite(head, 4, 2, o);
	fwrite(n.data(), 4, S, o);
	for (int v = 0; v < S; ++v) fwrite(list.data() + (size_t)v * cap, 4, n[v], o);
	fclose(o);
	printf("%lld checks ok\n", checks);
	return 0;
}
