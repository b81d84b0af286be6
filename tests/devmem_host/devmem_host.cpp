// devmem_host.cpp — TEST INFRASTRUCTURE: csrc/dvp_devmem.hpp on the host.  Block<FakeMem> is DevBlock with a counting stand-in
// for hipMalloc / hipFree that can be told to refuse the k-th request or every request above a size; Carve is checked against the
// take() arithmetic that labels_reserve and dvpprior::reserve spelled out before they shared it.
//   devmem_host                                  the block scenarios, and the layouts of the built-in geometries
//   devmem_host labels W H scale                 ... and of one label geometry
//   devmem_host prior cols rows W H tris rows    ... and of one plane-prior geometry
// (any number of such groups).  Prints "<n> checks ok"; a failed check prints its line and exits 1.
#define DVP_DEVMEM_NO_HIP
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <utility>
#include <vector>

#include "../../dvp-mvs_amd/csrc/dvp_devmem.hpp"
#include "../../dvp-mvs_amd/csrc/dvp_labels.hpp"
#include "../../dvp-mvs_amd/csrc/dvp_prior.hpp"

static long g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct FakeMem {
	using Stream = int*;   // a wait adds one to what it points to
	static std::map<void*, size_t> live;
	static long requests, frees, double_frees;
	static long refuse_nth;        // 1-based count of the request to refuse, 0 = none
	static size_t refuse_above;    // refuse every request larger than this, 0 = none
	static void reset() { requests = frees = double_frees = 0; refuse_nth = 0; refuse_above = 0; }
	static void* alloc(size_t bytes) {
		++requests;
		if ((refuse_nth && requests == refuse_nth) || (refuse_above && bytes > refuse_above)) return nullptr;
		void* p = malloc(bytes ? bytes : 1);   // (freed by free(): the address sanitizer sees a leak or a double free of its own)
		live[p] = bytes;
		return p;
	}
	static void free(void* p) {
		++frees;
		if (!live.erase(p)) { ++double_frees; return; }
		::free(p);
	}
	static int wait(Stream s) { ++*s; return 0; }
};
std::map<void*, size_t> FakeMem::live;
long FakeMem::requests, FakeMem::frees, FakeMem::double_frees, FakeMem::refuse_nth;
size_t FakeMem::refuse_above;

using Block = dvpmem::Block<FakeMem>;

static void end_of_scenario() {
	CHECK(FakeMem::live.empty());
	CHECK(FakeMem::double_frees == 0);
	FakeMem::reset();
}

static void block_scenarios() {
	FakeMem::reset();
	unsetenv("DVP_TEST_SIDE_ALLOC_FAIL");
	{   // grow-only: a smaller reserve after a larger keeps the pointer; an equal one too; 0 bytes never allocates
		Block b;
		CHECK(b.capacity() == 0 && b.as<char>() == nullptr);
		CHECK(b.reserve(0) == 0 && !b.as<void>() && FakeMem::requests == 0);
		CHECK(b.reserve(1000) == 0 && b.as<void>() && b.capacity() == 1000);
		char* p = b.as<char>();
		memset(p, 7, 1000);
		CHECK(b.reserve(10) == 0 && b.as<char>() == p && b.capacity() == 1000);
		CHECK(b.reserve(1000) == 0 && b.as<char>() == p);
		CHECK(b.reserve(0) == 0 && b.as<char>() == p);
		CHECK(FakeMem::requests == 1 && FakeMem::frees == 0);
		CHECK(b.reserve(1001) == 0 && b.capacity() == 1001 && FakeMem::requests == 2 && FakeMem::frees == 1 && FakeMem::live.size() == 1);
		memset(b.as<char>(), 7, 1001);
	}
	CHECK(FakeMem::frees == 2);   // the destructor frees
	end_of_scenario();
	{   // the wait runs before a regrow frees the old block, and only then
		int waits = 0;
		Block b;
		CHECK(b.reserve(64, &waits) == 0 && waits == 0);   // nothing to free yet
		CHECK(b.reserve(32, &waits) == 0 && waits == 0);   // fits
		CHECK(b.reserve(65, &waits) == 0 && waits == 1);
		CHECK(b.reserve(66) == 0 && waits == 1);           // no stream given
	}
	end_of_scenario();
	{   // a refused reserve (the k-th request) leaves the block empty and frees the old block exactly once
		Block b;
		CHECK(b.reserve(100) == 0);
		FakeMem::refuse_nth = 2;
		CHECK(b.reserve(200) != 0);
		CHECK(b.capacity() == 0 && b.as<void>() == nullptr);
		CHECK(FakeMem::frees == 1 && FakeMem::live.empty());
		b.release();   // releasing an empty block frees nothing
		CHECK(FakeMem::frees == 1);
		CHECK(b.reserve(50) == 0 && b.capacity() == 50);   // and it can be used again
	}
	CHECK(FakeMem::frees == 2);
	end_of_scenario();
	{   // a refusal by size: the smaller block of a pair stands, the larger is refused; an empty block stays empty
		FakeMem::refuse_above = 4096;
		Block a, b;
		CHECK(a.reserve(4096) == 0 && b.reserve(4097) != 0 && a.as<void>() && !b.as<void>());
		CHECK(b.reserve(4097) != 0 && !b.as<void>() && b.capacity() == 0 && FakeMem::frees == 0);
	}
	end_of_scenario();
	{   // DVP_TEST_SIDE_ALLOC_FAIL=N refuses every request of at least N bytes before the allocator sees it, and frees the old block
		Block b;
		CHECK(b.reserve(100) == 0);
		setenv("DVP_TEST_SIDE_ALLOC_FAIL", "128", 1);
		CHECK(b.reserve(127) == 0 && FakeMem::requests == 2);
		CHECK(b.reserve(128) != 0 && !b.as<void>() && b.capacity() == 0 && FakeMem::requests == 2 && FakeMem::frees == 2 && FakeMem::live.empty());
		CHECK(b.reserve(0) == 0);   // nothing is asked for
		setenv("DVP_TEST_SIDE_ALLOC_FAIL", "1", 1);
		CHECK(b.reserve(1) != 0);
		unsetenv("DVP_TEST_SIDE_ALLOC_FAIL");
		CHECK(b.reserve(128) == 0 && b.capacity() == 128);
	}
	end_of_scenario();
	{   // move leaves the source empty; move assignment frees what the target held; release() empties
		Block a;
		CHECK(a.reserve(300) == 0);
		void* p = a.as<void>();
		Block b(std::move(a));
		CHECK(!a.as<void>() && a.capacity() == 0 && b.as<void>() == p && b.capacity() == 300);
		Block c;
		CHECK(c.reserve(20) == 0);
		c = std::move(b);
		CHECK(!b.as<void>() && b.capacity() == 0 && c.as<void>() == p && c.capacity() == 300 && FakeMem::frees == 1 && FakeMem::live.size() == 1);
		c = std::move(c);   // (self-assignment keeps the block)
		CHECK(c.as<void>() == p);
		std::vector<Block> v;
		v.push_back(std::move(c));
		for (int i = 0; i < 20; ++i) { Block d; CHECK(d.reserve(8 + i) == 0); v.push_back(std::move(d)); }   // the vector regrows by moving
		CHECK(v[0].as<void>() == p && FakeMem::live.size() == 21);
		v[0].release();
		CHECK(!v[0].as<void>() && v[0].capacity() == 0 && FakeMem::live.size() == 20);
	}
	end_of_scenario();
	{   // CallError
		dvpmem::CallError e;
		CHECK(e.fail("who", "what") == 1 && e.text == "who: what" && strcmp(e.c_str(), "who: what") == 0);
		CHECK(e.fail(nullptr, "what alone") == 1 && e.text == "what alone");
		e.clear();
		CHECK(e.text.empty());
	}
}

// ---- the layouts as the two stages computed them before dvpmem::Carve -------------------------------------------------------
struct OldTake {
	size_t at = 0;
	size_t take(size_t bytes) { const size_t here = at; at += (bytes + 255) & ~(size_t)255; return here; }
};

static void labels_layout(int W, int H, int scale) {
	const dvplab::Geometry g = dvplab::geometry(W, H, scale);
	const size_t Lf = (size_t)g.W * g.H, Lh = (size_t)g.hw * g.hh, Lq = (size_t)g.qw * g.qh, Ll = (size_t)g.lw * g.lh, Lm = Lq > Ll ? Lq : Ll;
	const size_t blocks = (Ll + dvplab::SCAN_BLOCK - 1) / dvplab::SCAN_BLOCK;
	const size_t parts[13] = { Lf, Lh, Lq, Lq, Lq, Lq * 4, Lm * 4, Lq * 4, Ll, Ll, Ll * 4, Ll * 4, (blocks + 1) * 4 };   // labels_reserve's order
	OldTake o;
	dvpmem::Carve c;
	size_t end = 0;
	for (size_t bytes : parts) {
		const size_t want = o.take(bytes), got = c.take(bytes);
		CHECK(got == want && got % 256 == 0 && got >= end);   // aligned, and past the part before
		end = got + bytes;
	}
	CHECK(c.total == o.at && c.total >= end && c.total % 256 == 0);
}

static void prior_layout(size_t cols, size_t rows, size_t W, size_t H, size_t triangles, size_t sweep_rows) {
	const size_t Ld = cols * rows, Lw = W * H;
	const size_t parts[7] = { Ld * 4, Ld * 4, Ld * 4, Lw * 4, (triangles + 1) * sizeof(dvpprior::Tri), (triangles + 1) * 4, (sweep_rows + 1) * 4 };   // dvpprior::reserve's order
	OldTake o;
	dvpmem::Carve c;
	size_t end = 0;
	for (size_t bytes : parts) {
		const size_t want = o.take(bytes), got = c.take(bytes);
		CHECK(got == want && got % 256 == 0 && got >= end);
		end = got + bytes;
	}
	CHECK(c.total == o.at && c.total >= end && c.total % 256 == 0);
}

int main(int argc, char** argv) {
	block_scenarios();
	{   // Carve itself: nothing taken, empty parts, sizes on either side of the alignment
		dvpmem::Carve c;
		CHECK(c.total == 0);
		CHECK(c.take(0) == 0 && c.total == 0);
		CHECK(c.take(1) == 0 && c.total == 256);
		CHECK(c.take(256) == 256 && c.total == 512);
		CHECK(c.take(257) == 512 && c.total == 1024);
		CHECK(c.take(255) == 1024 && c.total == 1280);
	}
	// the sizes and scales of tests/np_labels.py, the map and working sizes of tests/np_prior.py with lists from none to long
	const int sizes[8][2] = { { 12, 12 }, { 13, 15 }, { 63, 65 }, { 130, 70 }, { 257, 131 }, { 258, 130 }, { 480, 360 }, { 515, 259 } };
	for (const auto& s : sizes)
		for (int scale = 0; scale <= 2; ++scale) labels_layout(s[0], s[1], scale);
	const int prior[4][4] = { { 96, 72, 96, 72 }, { 200, 100, 96, 72 }, { 191, 143, 96, 72 }, { 400, 300, 400, 300 } };
	for (const auto& p : prior)
		for (size_t t : { (size_t)0, (size_t)1, (size_t)4, (size_t)9, (size_t)1000 })
			for (size_t r : { (size_t)0, (size_t)63, (size_t)64, (size_t)3000, (size_t)100000 }) prior_layout(p[0], p[1], p[2], p[3], t, r);
	for (int i = 1; i < argc;) {
		if (!strcmp(argv[i], "labels") && i + 3 < argc) {
			labels_layout(atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]));
			i += 4;
		} else if (!strcmp(argv[i], "prior") && i + 6 < argc) {
			prior_layout(strtoull(argv[i + 1], nullptr, 10), strtoull(argv[i + 2], nullptr, 10), strtoull(argv[i + 3], nullptr, 10), strtoull(argv[i + 4], nullptr, 10),
			             strtoull(argv[i + 5], nullptr, 10), strtoull(argv[i + 6], nullptr, 10));
			i += 7;
		} else {
			printf("usage: devmem_host [labels W H scale | prior cols rows W H triangles sweep_rows]...\n");
			return 2;
		}
	}
	printf("%ld checks ok\n", g_checks);
	return 0;
}
