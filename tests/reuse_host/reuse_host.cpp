// Host check of the strong update's plane-cache plan (dvp_strong.hpp: strong_reuse_plan), the function dvp_strong_plan runs per
// pixel: seeded random old records and new slot sets, every property of the plan checked against a brute-force model.
// Stand-alone (own main) so that it can also be built with -fsanitize=address,undefined and run as a plain executable.
//   reuse_host [cases] [seed]      exit status 0 = all cases hold
#include "../../dvp-mvs_amd/csrc/dvp_strong.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace dvp;

static uint64_t g_state;
static uint32_t rnd() {   // xorshift64*
	g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
	return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static uint32_t rnd_below(uint32_t n) { return rnd() % n; }

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static bool same_key(const PlaneKey& a, const PlaneKey& b) { return std::memcmp(a.w, b.w, 16) == 0; }

// a pool of planes in which bitwise-distinct entries compare equal (or unordered) as floats: signs of zero, NaN payloads
constexpr int kPool = 40;
static PlaneKey g_pool[kPool];
static void make_pool() {
	const uint32_t specials[8] = { 0x00000000u, 0x80000000u, 0x7FC00000u, 0x7FC00001u, 0xFFC00000u, 0x7F800001u, 0x3F800000u, 0xBF800000u };
	for (int i = 0; i < kPool; ++i) {
		for (;;) {
			for (int k = 0; k < 4; ++k) {
				const uint32_t r = rnd();
				g_pool[i].w[k] = (r & 3u) ? specials[(r >> 2) & 7u] : f32_bits((float)((int)((r >> 8) & 15u) - 8) * 0.25f);
			}
			bool fresh = true;
			for (int j = 0; j < i; ++j) fresh = fresh && !same_key(g_pool[i], g_pool[j]);
			if (fresh) break;
		}
	}
}
static f4 plane_of(const PlaneKey& k) { return mk4(from_bits(k.w[0]), from_bits(k.w[1]), from_bits(k.w[2]), from_bits(k.w[3])); }

#define FAIL(...) do { std::fprintf(stderr, "case %ld: ", it); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } while (0)

int main(int argc, char** argv) {
	const long cases = argc > 1 ? std::atol(argv[1]) : 300000;
	g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 0x9E3779B97F4A7C15ull;
	if (!g_state) g_state = 1;
	make_pool();
	long hits_seen = 0, evals_seen = 0, stale_seen = 0, by_valid[kSlotCount + 1] = { 0 };
	for (long it = 0; it < cases; ++it) {
		// ---- the visit's slots: some missing, planes from a small part of the pool so that they repeat ----
		const int span = 1 + (int)rnd_below(kPool);
		const int base = (int)rnd_below(kPool);
		f4 pl[kSlotCount];
		PlaneKey want[kSlotCount];
		uint32_t have = 1u << kSlotCur;   // the current plane is always there
		const uint32_t miss_rate = rnd_below(4);   // 0: all slots present
		for (int s = 0; s < kSlotCount; ++s) {
			if (s < kSlotCur && !(miss_rate && rnd_below(4) < miss_rate)) have |= 1u << s;
			std::memset(&want[s], 0, sizeof(PlaneKey));
			pl[s] = mk4(0.0f, 0.0f, 0.0f, 0.0f);
			if ((have >> s) & 1u) { want[s] = g_pool[(base + (int)rnd_below((uint32_t)span)) % kPool]; pl[s] = plane_of(want[s]); }
		}
		for (int s = 0; s < kSlotCount; ++s)   // (copies of floats keep their bits, signalling NaNs included)
			if (!same_key(plane_key(pl[s]), want[s])) FAIL("plane_key does not round-trip slot %d", s);
		uint32_t src[3];
		const uint32_t uniq = strong_slot_sources_of(pl, have, src);
		// ---- the old record: 0..17 valid places with distinct keys, anything in the others ----
		const int nvalid = (int)rnd_below(kSlotCount + 1);
		by_valid[nvalid]++;
		uint32_t valid = 0;
		while (__builtin_popcount(valid) < nvalid) valid |= 1u << rnd_below(kSlotCount);
		PlaneKey keys[kSlotCount], old_keys[kSlotCount];
		for (int p = 0; p < kSlotCount; ++p) {
			for (int tries = 0;; ++tries) {   // near the visit's planes first, then anywhere in the pool (40 entries: 17 distinct ones exist)
				keys[p] = g_pool[tries < 20 ? (base + (int)rnd_below((uint32_t)(span + 6))) % kPool : (int)rnd_below(kPool)];
				bool fresh = true;
				if ((valid >> p) & 1u)
					for (int q = 0; q < p; ++q) fresh = fresh && !(((valid >> q) & 1u) && same_key(keys[p], keys[q]));
				if (fresh) break;
			}
			old_keys[p] = keys[p];
		}
		const uint32_t epoch = 1 + rnd_below(5), radius = 5 * (1 + rnd_below(3));
		ReuseHdr hdr;
		hdr.valid = valid | (rnd() & ~kPlaceMask);   // bits above the places are not places
		hdr.epoch = rnd_below(10) < 7 ? epoch : epoch + 1 + rnd_below(3);
		hdr.radius = rnd_below(10) < 7 ? radius : radius + 5;
		hdr.eval = rnd();
		const bool live = hdr.epoch == epoch && hdr.radius == radius;
		if (!live) stale_seen++;
		uint32_t pw[3];
		const uint32_t eval = strong_reuse_plan(pl, uniq, src, keys, &hdr, epoch, (int)radius, pw);
		// ---- model ----
		int place[kSlotCount];
		for (int s = 0; s < kSlotCount; ++s) place[s] = strong_slot_place_of(pw[0], pw[1], pw[2], s);
		if (hdr.epoch != epoch || hdr.radius != radius || hdr.eval != eval) FAIL("header not rewritten");
		if (eval & ~uniq) FAIL("evaluation mask %x outside uniq %x", eval, uniq);
		if (!live && eval != uniq) FAIL("(e) stale record, mask %x != uniq %x", eval, uniq);
		uint32_t used = 0, expect_eval = 0;
		for (int s = 0; s < kSlotCount; ++s) {
			if (!((have >> s) & 1u)) continue;
			const int p = place[s];
			if (p < 0 || p >= kSlotCount) FAIL("slot %d: place %d", s, p);
			used |= 1u << p;
			// (a) the place's key is the slot's plane
			if (!same_key(keys[p], want[s])) FAIL("(a) slot %d at place %d: key differs from the plane", s, p);
			// was the plane in the live record?
			int old_place = -1;
			if (live)
				for (int q = kSlotCount - 1; q >= 0; --q)
					if (((valid >> q) & 1u) && same_key(old_keys[q], want[s])) old_place = q;
			bool first = true;   // the earliest slot with this plane
			for (int u = 0; u < s; ++u) first = first && !(((have >> u) & 1u) && same_key(want[u], want[s]));
			if (old_place >= 0) {   // (b)
				if (p != old_place) FAIL("(b) slot %d: hit moved from place %d to %d", s, old_place, p);
				if ((eval >> s) & 1u) FAIL("(b) slot %d: hit is evaluated", s);
				if (!same_key(keys[p], old_keys[p])) FAIL("(b) slot %d: hit key rewritten", s);
				hits_seen += first;
			} else if (first) expect_eval |= 1u << s;   // (c)
			// (d) same place <=> same plane
			for (int u = 0; u < s; ++u)
				if (((have >> u) & 1u) && (place[u] == p) != same_key(want[u], want[s])) FAIL("(d) slots %d and %d: places %d / %d", u, s, place[u], p);
		}
		if (eval != expect_eval) FAIL("(c) mask %x, expected one slot per missed plane %x", eval, expect_eval);
		evals_seen += __builtin_popcount(eval);
		if (hdr.valid != used) FAIL("valid places %x, used %x", hdr.valid, used);
		// a miss takes the lowest place no hit holds, in increasing slot order; nothing else is written
		{
			uint32_t held = 0;
			for (int s = 0; s < kSlotCount; ++s)
				if (((uniq >> s) & 1u) && !((eval >> s) & 1u)) held |= 1u << place[s];
			uint32_t free_places = kPlaceMask & ~held;
			for (int s = 0; s < kSlotCount; ++s)
				if ((eval >> s) & 1u) {
					if (place[s] != __builtin_ctz(free_places)) FAIL("miss slot %d at place %d, lowest free %d", s, place[s], __builtin_ctz(free_places));
					free_places &= free_places - 1;
				}
			for (int p = 0; p < kSlotCount; ++p)
				if (!((used >> p) & 1u) && !same_key(keys[p], old_keys[p])) FAIL("place %d written without a slot", p);
		}
	}
	for (int n = 0; n <= kSlotCount; ++n)
		if (cases >= 100000 && by_valid[n] == 0) { std::fprintf(stderr, "no case with %d valid places\n", n); return 1; }
	if (cases >= 100000 && (hits_seen == 0 || evals_seen == 0 || stale_seen == 0)) { std::fprintf(stderr, "degenerate case mix\n"); return 1; }
	std::printf("reuse_host: %ld cases ok (%ld hits, %ld evaluations, %ld stale records)\n", cases, hits_seen, evals_seen, stale_seen);
	return 0;
}
