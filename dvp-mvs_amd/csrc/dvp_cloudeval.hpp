// dvp_cloudeval.hpp — the definition behind `apd --evaluate`: nearest-neighbour distances between two point clouds, clipped at the
// largest tolerance, and the counts accuracy / completeness / F1 are made of.  The same text for the device (dvp_cloudeval.hip), the
// host flavour (host/evaluate.cpp) and the test tool (tests/cloudeval_host).
//   distance   m(p) = min over the targets q with three finite coordinates of (dx*dx + dy*dy) + dz*dz, d = p - q, binary32, one
//              rounding per operator (-ffp-contract=off).  d2(p) = m(p) if m(p) <= T2 else +inf, T2 = T*T in binary32, T the largest
//              tolerance.  A query with a non-finite coordinate gets NaN and is in no count.  No finite target: +inf everywhere.
//   counts     within[k] = finite-coordinate queries with d2 <= t_k*t_k (binary32 product), used = finite-coordinate queries.
//   grid       one uniform grid over both clouds: edge h = (double)T * (1 + 2^-10), origin = per-axis minimum over the finite points of
//              both clouds, cell index floor(((double)x - origin) / h) in binary64.  A rounded d2 <= T2 implies a true per-axis
//              difference below T (1 + 2^-22) < h, so the nearest target of a query with a finite result lies in the 27 cells around
//              the query's cell ("Cloud evaluation").  min and integer sums do not depend on the order: the grid's answer
//              is the brute-force double loop's, bit for bit.
//   table      occupied cells in an open-addressing table: 64-bit keys (three 21-bit indices, each stored + 1 so that a neighbour's
//              index never borrows), capacity a power of two >= 2 x the points binned, linear probing from hash_key(key).  At most
//              2^30 points are binned (the finite points of both clouds together): a slot then fits 32 bits.
#ifndef DVP_CLOUDEVAL_HPP_
#define DVP_CLOUDEVAL_HPP_

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define DVP_CHD __host__ __device__ inline
#else
#define DVP_CHD inline
#endif

#include <string>
#include <vector>

namespace dvpce {

constexpr int kMaxTolerances = 8;
constexpr long long kMaxPoints = 2147483647ll;            // per cloud
constexpr long long kMaxBinned = 1ll << 30;               // finite points of both clouds together: the table then has at most 2^31 slots, and a
                                                          // slot fits the 32 bits it is kept in per point, clear of the "not binned" mark
constexpr long long kMaxCellsPerAxis = (1ll << 21) - 2;   // indices 1 ... 2^21 - 2 are stored, 0 and 2^21 - 1 only ever looked up
constexpr uint64_t kEmptyKey = ~0ull;                     // (no key has bit 63 set)
constexpr long long kBruteForcePairs = 1ll << 24;         // the host flavour runs the double loop up to this many (query, target) pairs

struct Grid {
	double origin[3];
	double h;
};

DVP_CHD bool finite3(float x, float y, float z) {
	// x - x is 0 for a finite x and NaN otherwise
	return (x - x) == 0.0f && (y - y) == 0.0f && (z - z) == 0.0f;
}

DVP_CHD float sq_dist(float px, float py, float pz, float qx, float qy, float qz) {
	const float dx = px - qx, dy = py - qy, dz = pz - qz;
	return (dx * dx + dy * dy) + dz * dz;
}

// NaN compares false: `best` is only ever replaced by a smaller number
DVP_CHD float keep_min(float best, float d) { return d < best ? d : best; }

DVP_CHD float clipped(float m, float T2) { return m <= T2 ? m : INFINITY; }

DVP_CHD uint64_t axis_index(double x, double origin, double h) { return (uint64_t)floor((x - origin) / h) + 1u; }

DVP_CHD uint64_t cell_key(const Grid& g, float x, float y, float z) {
	return (axis_index((double)x, g.origin[0], g.h) << 42) | (axis_index((double)y, g.origin[1], g.h) << 21) | axis_index((double)z, g.origin[2], g.h);
}

// the key of neighbour n = 0 ... 26 of a stored cell (13 = the cell itself): every stored index is >= 1 and <= 2^21 - 2
DVP_CHD uint64_t neighbour_key(uint64_t key, int n) {
	const int64_t dx = n / 9 - 1, dy = (n / 3) % 3 - 1, dz = n % 3 - 1;
	return (uint64_t)((int64_t)key + dx * ((int64_t)1 << 42) + dy * ((int64_t)1 << 21) + dz);
}

// the home slot of a cell is hash_key(key) & (capacity - 1)   (the finaliser of splitmix64)
DVP_CHD uint64_t hash_key(uint64_t k) {
	k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
	k ^= k >> 27; k *= 0x94d049bb133111ebull;
	k ^= k >> 31;
	return k;
}

#if defined(__HIPCC__)
// the slot of `key`, or mask + 1
__device__ inline uint64_t find_slot(const unsigned long long* __restrict__ keys, uint64_t mask, uint64_t key) {
	for (uint64_t s = hash_key(key) & mask;; s = (s + 1) & mask) {
		const unsigned long long cur = keys[s];
		if (cur == key) return s;
		if (cur == kEmptyKey) return mask + 1;
	}
}
#endif

inline uint64_t table_capacity(uint64_t points) {
	uint64_t cap = 64;
	while (cap < 2 * points) cap <<= 1;
	return cap;
}

// ---- host part: argument checks, the grid of two clouds, the serial text ---------------------------------------------------------

// "" or what is wrong with the tolerances
inline std::string check_tolerances(const float* tol, int num_tol) {
	if (num_tol < 1 || num_tol > kMaxTolerances) return "num_tol must be 1 ... 8, got " + std::to_string(num_tol);
	char text[160];
	for (int k = 0; k < num_tol; ++k) {
		const float t = tol[k], t2 = t * t;
		if (!(t > 0.0f) || !((t - t) == 0.0f) || !((t2 - t2) == 0.0f) || t2 < 1.17549435e-38f) {
			snprintf(text, sizeof text, "tolerance %d (%.9g) must be finite and positive with a normal binary32 square", k, (double)t);
			return text;
		}
		if (k > 0 && !(tol[k - 1] < t)) {
			snprintf(text, sizeof text, "the tolerances must be strictly ascending, %.9g follows %.9g", (double)t, (double)tol[k - 1]);
			return text;
		}
	}
	return "";
}

struct Bounds {
	float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	long long finite = 0;
	void add(const float* xyz, long long n) {
		for (long long i = 0; i < n; ++i) {
			const float* p = xyz + 3 * i;
			if (!finite3(p[0], p[1], p[2])) continue;
			++finite;
			for (int a = 0; a < 3; ++a) {
				if (p[a] < lo[a]) lo[a] = p[a];
				if (p[a] > hi[a]) hi[a] = p[a];
			}
		}
	}
};

// "" or why `finite` points cannot be binned into one table
inline std::string check_binned(long long finite) {
	if (finite <= kMaxBinned) return "";
	return "the two clouds hold " + std::to_string(finite) + " points with finite coordinates together; at most " + std::to_string(kMaxBinned) + " (2^30) are supported";
}

// the grid over the finite points within `b`; "" or the error: too many points for one table, or the extent
inline std::string make_grid(const Bounds& b, float T, Grid* g) {
	const std::string many = check_binned(b.finite);
	if (!many.empty()) return many;
	g->h = (double)T * (1.0 + 1.0 / 1024.0);
	for (int a = 0; a < 3; ++a) g->origin[a] = b.finite ? (double)b.lo[a] : 0.0;
	for (int a = 0; a < 3 && b.finite; ++a) {
		const double cells = floor(((double)b.hi[a] - g->origin[a]) / g->h) + 1.0;
		if (!(cells <= (double)kMaxCellsPerAxis)) {
			char text[240];
			snprintf(text, sizeof text, "the clouds extend over %.9g along axis %d, which is %.0f cells of the largest tolerance %.9g; at most %lld are supported",
			         (double)b.hi[a] - g->origin[a], a, cells, (double)T, kMaxCellsPerAxis);
			return text;
		}
	}
	return "";
}

// The occupied cells of one cloud on the host, built the way the device builds them: claim a slot, count, exclusive prefix, scatter.
struct HostCells {
	uint64_t cap = 0;
	std::vector<uint64_t> keys;
	std::vector<uint32_t> start;    // cap + 1
	std::vector<uint32_t> index;    // point indices, cell after cell
	uint64_t find(uint64_t key) const {   // the slot of `key`, or cap
		for (uint64_t s = hash_key(key) & (cap - 1);; s = (s + 1) & (cap - 1)) {
			if (keys[s] == key) return s;
			if (keys[s] == kEmptyKey) return cap;
		}
	}
	void build(const Grid& g, const float* xyz, long long n, uint64_t capacity) {
		cap = capacity;
		keys.assign(cap, kEmptyKey);
		start.assign(cap + 1, 0u);
		std::vector<uint32_t> slot_of((size_t)n, 0xffffffffu);
		for (long long i = 0; i < n; ++i) {
			const float* p = xyz + 3 * i;
			if (!finite3(p[0], p[1], p[2])) continue;
			const uint64_t key = cell_key(g, p[0], p[1], p[2]);
			uint64_t s = hash_key(key) & (cap - 1);
			while (keys[s] != key && keys[s] != kEmptyKey) s = (s + 1) & (cap - 1);
			keys[s] = key;
			++start[s + 1];
			slot_of[(size_t)i] = (uint32_t)s;
		}
		for (uint64_t s = 0; s < cap; ++s) start[s + 1] += start[s];
		index.assign(start[cap], 0u);
		std::vector<uint32_t> cursor(start.begin(), start.end() - 1);
		for (long long i = 0; i < n; ++i)
			if (slot_of[(size_t)i] != 0xffffffffu) index[cursor[slot_of[(size_t)i]]++] = (uint32_t)i;
	}
};

// d2_out[i] of every query against the target cloud: the double loop (`brute`), or the grid walked serially
inline void serial_distances(const Grid& g, const float* query, long long nq, const float* target, long long nt, float T, bool brute, float* d2_out) {
	const float T2 = T * T;
	HostCells cells;
	if (!brute) {
		long long finite = 0;
		for (long long j = 0; j < nt; ++j) finite += finite3(target[3 * j], target[3 * j + 1], target[3 * j + 2]);
		cells.build(g, target, nt, table_capacity((uint64_t)finite));
	}
	for (long long i = 0; i < nq; ++i) {
		const float* p = query + 3 * i;
		if (!finite3(p[0], p[1], p[2])) { d2_out[i] = NAN; continue; }
		float best = INFINITY;
		if (brute) {
			for (long long j = 0; j < nt; ++j) {
				const float* q = target + 3 * j;
				if (finite3(q[0], q[1], q[2])) best = keep_min(best, sq_dist(p[0], p[1], p[2], q[0], q[1], q[2]));
			}
		} else {
			const uint64_t key = cell_key(g, p[0], p[1], p[2]);
			for (int n = 0; n < 27; ++n) {
				const uint64_t s = cells.find(neighbour_key(key, n));
				if (s == cells.cap) continue;
				for (uint32_t at = cells.start[s]; at < cells.start[s + 1]; ++at) {
					const float* q = target + 3 * (size_t)cells.index[at];
					best = keep_min(best, sq_dist(p[0], p[1], p[2], q[0], q[1], q[2]));
				}
			}
		}
		d2_out[i] = clipped(best, T2);
	}
}

// within[k] and *used from the distances of one direction
inline void count_within(const float* d2, long long n, const float* tol, int num_tol, long long* within, long long* used) {
	for (int k = 0; k < num_tol; ++k) within[k] = 0;
	*used = 0;
	for (long long i = 0; i < n; ++i) {
		if (d2[i] != d2[i]) continue;
		++*used;
		for (int k = 0; k < num_tol; ++k) within[k] += d2[i] <= tol[k] * tol[k];
	}
}

// both directions on the host; "" or the error.  d2_recon / d2_truth may be NULL.
inline std::string serial_evaluate(const float* recon, long long nr, const float* truth, long long nt, const float* tol, int num_tol, long long* within_recon,
                                   long long* within_truth, long long* used, float* d2_recon, float* d2_truth) {
	const std::string what = check_tolerances(tol, num_tol);
	if (!what.empty()) return what;
	const float T = tol[num_tol - 1];
	Bounds b;
	b.add(recon, nr);
	b.add(truth, nt);
	Grid g;
	const std::string extent = make_grid(b, T, &g);
	if (!extent.empty()) return extent;
	const bool brute = nr * nt <= kBruteForcePairs;
	std::vector<float> a((size_t)nr), c((size_t)nt);
	serial_distances(g, recon, nr, truth, nt, T, brute, a.data());
	serial_distances(g, truth, nt, recon, nr, T, brute, c.data());
	count_within(a.data(), nr, tol, num_tol, within_recon, &used[0]);
	count_within(c.data(), nt, tol, num_tol, within_truth, &used[1]);
	if (d2_recon) for (long long i = 0; i < nr; ++i) d2_recon[i] = a[(size_t)i];
	if (d2_truth) for (long long i = 0; i < nt; ++i) d2_truth[i] = c[(size_t)i];
	return "";
}

}   // namespace dvpce
#endif
