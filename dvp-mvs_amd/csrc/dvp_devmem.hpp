// dvp_devmem.hpp — the one place that owns the side stages' device memory (edges, view clean-up, labels, level images, plane prior,
// previews, fusion; the engine's context arena — dalloc, dfree, alloc_group_or_fall_back — has its own rule and is not here):
//   DevBlock     move-only owner of one device allocation that only grows
//   Carve        the layout of one block's parts, 256-byte aligned                                    (no HIP in it)
//   StreamScope  the stream of a one-shot "host in, host out" call
//   CallError    the text behind a unit's *_last_error
// The allocation calls sit behind the template parameter of Block: a host program defines DVP_DEVMEM_NO_HIP, includes this file
// without any HIP header and instantiates Block with a counting stand-in (tests/devmem_host).
#ifndef DVP_DEVMEM_HPP_
#define DVP_DEVMEM_HPP_

#include <stddef.h>
#include <stdlib.h>

#include <string>

#ifndef DVP_DEVMEM_NO_HIP
#include <hip/hip_runtime.h>
#endif

namespace dvpmem {

// Mem::alloc(bytes) -> pointer or NULL (a refusal leaves no status behind), Mem::free(pointer), Mem::wait(stream) -> non-zero on failure
template <class Mem>
class Block {
public:
	Block() = default;
	Block(Block&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	Block& operator=(Block&& o) noexcept {   // (the deleted copies follow from the declared moves)
		if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
		return *this;
	}
	~Block() { release(); }

	// Grow-only: 0 at once when the capacity suffices (a request of 0 bytes always does).  Otherwise the old block is freed — after
	// a wait for `stream` when one is given: work queued there may still use it — and a new one of exactly `bytes` is made.
	// Non-zero: out of device memory — the block is then empty, and HIP's sticky status clear — or the wait failed, which leaves
	// the block as it was.
	// DVP_TEST_SIDE_ALLOC_FAIL=N refuses every request of at least N bytes (read at each request, like the engine's
	// DVP_TEST_*_ALLOC_FAIL hooks).
	int reserve(size_t bytes, typename Mem::Stream stream = nullptr) {
		if (bytes <= cap_) return 0;
		if (p_ && stream && Mem::wait(stream)) return 1;
		release();
		const char* hook = getenv("DVP_TEST_SIDE_ALLOC_FAIL");
		if (hook && bytes >= strtoull(hook, nullptr, 10)) return 1;
		p_ = Mem::alloc(bytes);
		if (!p_) return 1;
		cap_ = bytes;
		return 0;
	}
	void release() { if (p_) Mem::free(p_); p_ = nullptr; cap_ = 0; }
	template <class T>
	T* as() const { return static_cast<T*>(p_); }
	size_t capacity() const { return cap_; }

private:
	void* p_ = nullptr;
	size_t cap_ = 0;
};

// offsets of a block's parts in the order they are taken, each on a 256-byte boundary; `total` is the block's size
struct Carve {
	size_t total = 0;
	size_t take(size_t bytes) { const size_t here = total; total += (bytes + 255) & ~(size_t)255; return here; }
};

// one thread-local instance per unit: the C ABI has one *_last_error per unit
struct CallError {
	std::string text;
	void clear() { text.clear(); }
	const char* c_str() const { return text.c_str(); }
	// "who: what", or what alone when who is NULL; returns 1
	int fail(const char* who, const std::string& what) { text = who ? std::string(who) + ": " + what : what; return 1; }
};

#ifndef DVP_DEVMEM_NO_HIP
struct HipMem {
	using Stream = hipStream_t;
	static void* alloc(size_t bytes) {
		void* p = nullptr;
		if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		return p;
	}
	static void free(void* p) { (void)hipFree(p); }
	static int wait(hipStream_t s) { if (hipStreamSynchronize(s) == hipSuccess) return 0; (void)hipGetLastError(); return 1; }
};
using DevBlock = Block<HipMem>;

// The non-blocking stream of a one-shot call.  Declare it AFTER the (still empty) blocks the call uses: locals are destroyed in
// reverse order, so on every exit path its destructor waits for the stream and destroys it first, and the blocks are freed with
// nothing queued on them.
struct StreamScope {
	hipStream_t s = nullptr;
	StreamScope() = default;
	StreamScope(const StreamScope&) = delete;
	~StreamScope() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
	int open() {   // non-zero: hipStreamCreate failed
		if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess) return 0;
		(void)hipGetLastError(); s = nullptr; return 1;
	}
	operator hipStream_t() const { return s; }
};
#endif

}   // namespace dvpmem
#endif
