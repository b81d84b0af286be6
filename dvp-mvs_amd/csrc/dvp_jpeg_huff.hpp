// dvp_jpeg_huff.hpp — the Huffman scan of an input JPEG decoded in parallel (`apd --entropy-on gpu`): the per-lane arithmetic as
// __host__ __device__ functions.  The kernels of dvp_jpeg_huff.hip run them a lane per subsequence, the host emulation
// (tests/jpeg_huff_host) lane after lane in either order: one text, one result.  What leaves is what the serial scan of
// dvp_jpeg_dec_mid.hpp leaves — per component the raster-order `offsets` and `records` — or a raised flag, and then the serial scan
// is run instead: a result that differs from the serial one does not exist.
//
// A Huffman stream self-synchronises (Klein and Wiseman 2003): a decoder that starts at a wrong place decodes rubbish for a while
// and then, with high probability, falls into step with the right one.  The scheme (Weissenberger and Schmidt 2021):
//   segments      the stretches of entropy-coded bytes between RSTn markers; every segment starts a fresh bit stream and fresh
//                 DC predictions, and holds a known quota of MCUs
//   subsequences  a segment cut, from its own first byte, into pieces of `subseq_bytes` STUFFED bytes; a lane owns one
//   state         (bit position in the segment, block within the MCU, zig-zag index) at the start of a symbol — a symbol is a
//                 Huffman code with the value bits that follow it.  Positions count stuffed bytes, and are canonical: never
//                 inside or at a stuffed zero
//   entry state   st[lane]: lane 0 of a segment starts exact at (0, 0, 0); every other lane from the guess "a block begins at my
//                 first byte"
//   synchronise   a lane decodes its subsequence and runs on into the next ones; after each it compares its state with the entry
//                 state stored there, stops when they are equal (its trajectory has merged with the one that wrote it) and stores
//                 its own otherwise.  Inside a chunk of kChunkLanes lanes this is one kernel with a barrier per step; across chunk
//                 boundaries the states travel through carry[] in rounds that the host repeats while a state changed
//   census        every lane decodes from its final entry state, checks that it leaves in the next lane's entry state, and counts
//                 the blocks that BEGIN in its subsequence: those are the lane's own, and it decodes them to their end, wherever
//                 that lies.  By induction from lane 0 the check alone proves every state exact, whatever the synchronisation did
//   count         (after a prefix sum of the census: the lane knows its first block's number in the segment) records per block
//                 and the DC difference per block; corrupt codes and a segment that does not hold exactly its quota raise the flag
//   scans         offsets = prefix sum of the counts in raster order; DC predictions = prefix sum of the differences in scan order
//                 per component, restarted at every segment
//   write         make_record(position, value) at offsets[block], directly in raster order
// A speculative trajectory that meets an invalid code or a run past 63 does not stop — it would hand its error state down the
// whole file, one subsequence per step.  It drops the code (an invalid one) or ends the block (a run past 63) and goes on.
// Every loop is bounded by the bits of a subsequence plus one block's, the lanes of a chunk, or the round cap: nothing a file says
// makes a lane spin.  Every read of the bytes is checked against the segment; past its end the reader feeds zeros, as the serial
// reader does at a marker.
#ifndef DVP_JPEG_HUFF_HPP_
#define DVP_JPEG_HUFF_HPP_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DVP_JH_HD __host__ __device__
#else
#define DVP_JH_HD
#endif

namespace dvpjh {

constexpr int kChunkLanes = 256;         // subsequences per chunk = lanes per work-group of the synchronisation
constexpr int kRoundCap = 8;             // inter-chunk rounds before the path gives up
constexpr int kSubseqBytes = 128;        // (measured against 256 on the 25-Mpx file: DESIGN.md §7)
constexpr int kMaxMcuBlocks = 10;
constexpr int kBlockBitsMax = 2048;      // a block is at most 1 + 63 symbols of at most 16 + 15 bits: 1980
constexpr uint32_t kSegmentBytesMax = 1u << 28;
constexpr long long kDcLimit = 1 << 25;  // dvpjdmid::kValueLimit

// a Huffman table as the serial decoder walks it (dvpjdmid::Huff without the counts)
struct Table {
	int mincode[17], maxcode[17], valptr[17];
	uint8_t vals[256];
};
struct Tables {
	Table t[8];   // 0 ... 3: DC, 4 ... 7: AC
	uint8_t zigzag[64];
};

struct CompLayout {
	int h, v, hv, blocks_w, dc, ac, want, first_blk;   // dc, ac: indices into Tables::t; first_blk: its first block within the MCU
};
struct Layout {
	int comps, mcu_blocks, mcus_x, total_mcus, interval;   // interval: MCUs per segment (the whole scan when the file has no DRI)
	uint8_t blk_comp[kMaxMcuBlocks];
	CompLayout c[3];
};

struct Seg {
	uint32_t start, len;          // in the uploaded bytes
	uint32_t first_lane, lanes;
};

struct State {
	uint32_t p;    // bit position of the next symbol in the segment
	uint32_t bk;   // block within the MCU << 8 | zig-zag index (0: a block begins)
};
DVP_JH_HD inline unsigned long long pack(State s) { return ((unsigned long long)s.p << 32) | s.bk; }
DVP_JH_HD inline State unpack(unsigned long long w) { return State{ (uint32_t)(w >> 32), (uint32_t)w }; }

// counters[]: what the kernels report
enum { kFlag = 0, kChanged = 1, kLongest = 2, kDecodes = 3, kCounters = 4 };

// the arrays of one scan: device memory in the kernels, host memory in the emulation
struct Job {
	const uint8_t* bytes;
	const Seg* segs;
	const uint32_t* lane_seg;
	const Tables* tables;
	uint32_t lanes, segments, chunks;
	int subseq_bytes;
	unsigned long long* st;         // [lanes] entry states
	unsigned long long* carry[2];   // [chunks] the entry state of a chunk's first lane as the chunk before it left it
	uint32_t* began;                // [lanes] blocks that begin in the lane
	uint32_t* first_block;          // [lanes + 1] exclusive prefix sum of `began` over all lanes
	uint32_t* counters;
	Layout lay;
	uint32_t* offsets[3];           // [blocks + 1] per wanted component, else NULL; the count pass leaves block b's count at b + 1
	int32_t* dc[3];                 // [blocks] in the component's scan order: the differences, then (finish_dc) the predictions
	long long* dc_sum[3];           // [blocks] inclusive prefix sum of the differences
	uint32_t* records[3];
};

// ---- the bit reader over stuffed bytes ------------------------------------------------------------------------------------------
// Loads a byte at a time, and only when a bit is asked for: between two symbols the unread bits all lie in the byte loaded last,
// which gives the position without looking back.
struct Bits {
	const uint8_t* b;
	uint32_t len;
	uint32_t o, ol;   // the next byte to load; the byte loaded last
	uint32_t cur;
	int n;            // unread bits of `cur`
	DVP_JH_HD void load() {
		cur = o < len ? b[o] : 0u;
		ol = o;
		++o;
		if (cur == 0xFFu && o < len && b[o] == 0) ++o;   // the stuffed zero
		n = 8;
	}
	DVP_JH_HD void seek(uint32_t p) {
		o = p >> 3; ol = o; cur = 0; n = 0;
		const int used = (int)(p & 7u);
		if (used) { load(); n = 8 - used; }
	}
	DVP_JH_HD uint32_t pos() const { return n ? ol * 8u + (uint32_t)(8 - n) : o * 8u; }
	DVP_JH_HD int bit() { if (!n) load(); --n; return (int)((cur >> n) & 1u); }
	DVP_JH_HD int get(int count) {   // count <= 16
		int v = 0;
		while (count > 0) {
			if (!n) load();
			const int take = count < n ? count : n;
			v = (v << take) | (int)((cur >> (n - take)) & ((1u << take) - 1u));
			n -= take;
			count -= take;
		}
		return v;
	}
};

// where subsequence i of a segment begins: its first byte, or the one after it when that byte is the zero stuffed behind an 0xFF
DVP_JH_HD inline uint32_t first_position(const uint8_t* b, uint32_t len, uint32_t i, int subseq_bytes) {
	uint32_t o = i * (uint32_t)subseq_bytes;
	if (o > 0 && o < len && b[o] == 0 && b[o - 1] == 0xFF) ++o;
	return o * 8u;
}
DVP_JH_HD inline uint32_t end_position(uint32_t len, uint32_t i, int subseq_bytes) {
	const unsigned long long e = (unsigned long long)(i + 1) * (unsigned long long)subseq_bytes;
	return (uint32_t)(e < len ? e : len) * 8u;
}

// dvpjdmid::decode_symbol and dvpjdmid::extend
DVP_JH_HD inline int symbol(Bits& r, const Table& h) {
	int code = 0;
	for (int l = 1; l <= 16; ++l) {
		code = (code << 1) | r.bit();
		if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) return h.vals[h.valptr[l] + code - h.mincode[l]];
	}
	return -1;
}
DVP_JH_HD inline int extend(int v, int n) { return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v; }

// ---- one symbol -----------------------------------------------------------------------------------------------------------------
enum { kNone = 0, kDc = 1, kAc = 2 };
enum { kFine = 0, kBadDcCode = 1, kBadAcCode = 2, kBadAcRun = 3 };
struct Step {
	int kind;     // kDc: `value` is the DC difference; kAc: a coefficient `value` at zig-zag index `k`
	int k, value;
	int error;    // what the serial scan would have refused here
	bool block_end;
};

DVP_JH_HD inline void end_block(const Layout& lay, int& blk, int& k, Step& s) {
	s.block_end = true;
	k = 0;
	blk = blk + 1 == lay.mcu_blocks ? 0 : blk + 1;
}

// Decodes the symbol at the reader and moves (blk, k) on.  Consumes at least one bit, whatever it meets.
DVP_JH_HD inline Step step(Bits& r, const Tables& T, const Layout& lay, int& blk, int& k) {
	Step s = { kNone, 0, 0, kFine, false };
	const CompLayout& c = lay.c[lay.blk_comp[blk]];
	if (k == 0) {
		const int t = symbol(r, T.t[c.dc]);
		if (t < 0 || t > 11) s.error = kBadDcCode;   // (speculative: the code is dropped and the block goes on)
		else { s.kind = kDc; s.value = t ? extend(r.get(t), t) : 0; }
		k = 1;
		return s;
	}
	const int rs = symbol(r, T.t[4 + c.ac]);
	if (rs < 0) { s.error = kBadAcCode; return s; }   // (speculative: sixteen bits dropped)
	const int run = rs >> 4, size = rs & 15;
	if (size == 0) {
		if (run == 15) { k += 16; if (k >= 64) end_block(lay, blk, k, s); }
		else end_block(lay, blk, k, s);
		return s;
	}
	k += run;
	if (k > 63) { s.error = kBadAcRun; end_block(lay, blk, k, s); return s; }   // (speculative: the block ends)
	s.kind = kAc;
	s.k = k;
	s.value = extend(r.get(size), size);
	if (++k >= 64) end_block(lay, blk, k, s);
	return s;
}

// ---- "decode subsequence i from state s" ----------------------------------------------------------------------------------------
// From `s` to the first symbol that starts at or after end_bit; the state there.
DVP_JH_HD inline State run_subsequence(const uint8_t* b, uint32_t len, const Tables& T, const Layout& lay, State s, uint32_t end_bit, int subseq_bytes) {
	Bits r{ b, len, 0, 0, 0, 0 };
	r.seek(s.p);
	int blk = (int)(s.bk >> 8), k = (int)(s.bk & 255u);
	for (int n = 0; n < subseq_bytes * 8 && r.pos() < end_bit; ++n) (void)step(r, T, lay, blk, k);
	return State{ r.pos(), ((uint32_t)blk << 8) | (uint32_t)k };
}

// the state compare: false = equal, the trajectory has merged and its lane stops; true = stored, the lane goes on
DVP_JH_HD inline bool store_if_new(unsigned long long* slot, State s) {
	const unsigned long long w = pack(s);
	if (*slot == w) return false;
	*slot = w;
	return true;
}

// The blocks that begin in [entry, end_bit), each decoded to its end.  sink.begin(p) / sink.symbol(step) / sink.end(p after the
// block) see the lane's own blocks in order; what is left of a block that began before `entry` is passed over.  *leaves is the
// state at the first symbol at or after end_bit; false: the bound on the steps ran out (only rubbish is that long).
template <class Sink>
DVP_JH_HD inline bool run_blocks(const uint8_t* b, uint32_t len, const Tables& T, const Layout& lay, State entry, uint32_t end_bit, int subseq_bytes, Sink& sink, State* leaves) {
	Bits r{ b, len, 0, 0, 0, 0 };
	r.seek(entry.p);
	int blk = (int)(entry.bk >> 8), k = (int)(entry.bk & 255u);
	bool own = false, left = false;
	const int bound = subseq_bytes * 8 + kBlockBitsMax;
	for (int n = 0; n < bound; ++n) {
		const uint32_t p = r.pos();
		if (!left && p >= end_bit) { *leaves = State{ p, ((uint32_t)blk << 8) | (uint32_t)k }; left = true; }
		if (k == 0) {
			if (p >= end_bit) return true;   // the next lane's
			own = true;
			sink.begin(p, blk);
		} else if (!own && p >= end_bit) return true;
		const Step s = step(r, T, lay, blk, k);
		if (own) {
			sink.symbol(s);
			if (s.block_end) { sink.end(r.pos()); own = false; }
		}
	}
	return false;
}

// ---- where a block lies ---------------------------------------------------------------------------------------------------------
struct BlockPlace {
	int comp;
	uint32_t scan_index;     // in the component's scan order
	uint32_t raster_index;   // in the component's block raster
};
// block number `in_segment` of segment `seg`, whose MCU-block is `blk`
DVP_JH_HD inline BlockPlace place_of(const Layout& lay, uint32_t seg, uint32_t in_segment, int blk) {
	const uint32_t mcu = seg * (uint32_t)lay.interval + in_segment / (uint32_t)lay.mcu_blocks;
	const int ci = lay.blk_comp[blk];
	const CompLayout& c = lay.c[ci];
	const uint32_t w = (uint32_t)(blk - c.first_blk);
	const uint32_t my = mcu / (uint32_t)lay.mcus_x, mx = mcu % (uint32_t)lay.mcus_x;
	BlockPlace at;
	at.comp = ci;
	at.scan_index = mcu * (uint32_t)c.hv + w;
	at.raster_index = (my * (uint32_t)c.v + w / (uint32_t)c.h) * (uint32_t)c.blocks_w + mx * (uint32_t)c.h + w % (uint32_t)c.h;
	return at;
}
DVP_JH_HD inline uint32_t quota_blocks(const Layout& lay, uint32_t seg) {
	const long long left = (long long)lay.total_mcus - (long long)seg * lay.interval;
	return (uint32_t)(left < lay.interval ? left : lay.interval) * (uint32_t)lay.mcu_blocks;
}
// a segment's last block must end in the segment's last data byte: fewer than eight bits (the padding) are left over
DVP_JH_HD inline bool ends_the_segment(const uint8_t* b, uint32_t len, uint32_t p) {
	if (p == len * 8u) return true;
	const uint32_t last = len >= 2 && b[len - 1] == 0 && b[len - 2] == 0xFF ? len - 2 : len - 1;
	return p > last * 8u && p < last * 8u + 8u;
}

// ---- the lanes' passes ----------------------------------------------------------------------------------------------------------
struct LaneView {
	Seg sg;
	uint32_t seg, i;   // the segment's number; the lane's number inside it
	const uint8_t* b;
};
DVP_JH_HD inline LaneView lane_view(const Job& j, uint32_t lane) {
	LaneView v;
	v.seg = j.lane_seg[lane];
	v.sg = j.segs[v.seg];
	v.i = lane - v.sg.first_lane;
	v.b = j.bytes + v.sg.start;
	return v;
}

// before anything: the guesses
DVP_JH_HD inline void init_lane(const Job& j, uint32_t lane) {
	const LaneView v = lane_view(j, lane);
	const unsigned long long w = pack(State{ first_position(v.b, v.sg.len, v.i, j.subseq_bytes), 0u });
	j.st[lane] = w;
	if (lane % (uint32_t)kChunkLanes == 0) j.carry[0][lane / kChunkLanes] = j.carry[1][lane / kChunkLanes] = w;
}

// One step of the synchronisation inside a chunk for the lane that began at `lane`: (*at, *s) is the subsequence it stands
// before and the state it brings.  Returns whether the lane goes on; *carried: it stored a new state for the next chunk.
// Within a step no two lanes touch the same slot (they stand before different subsequences); between steps lies a barrier.
DVP_JH_HD inline bool sync_step(const Job& j, const Tables& T, uint32_t* at, State* s, bool* carried) {
	const LaneView v = lane_view(j, *at);
	*s = run_subsequence(v.b, v.sg.len, T, j.lay, *s, end_position(v.sg.len, v.i, j.subseq_bytes), j.subseq_bytes);
	if (v.i + 1 == v.sg.lanes) return false;   // the segment ends
	const uint32_t next = *at + 1;
	if (next % (uint32_t)kChunkLanes == 0) {
		if (store_if_new(&j.carry[0][next / kChunkLanes], *s)) *carried = true;
		return false;
	}
	*at = next;
	return store_if_new(&j.st[next], *s);
}

// One inter-chunk round for chunk c: reads carry[from], writes carry[1 - from][c + 1].  A chunk whose first lane has a new entry
// state walks that single trajectory through the chunk until it merges.  Returns the subsequences decoded; *carried as above.
DVP_JH_HD inline uint32_t round_chunk(const Job& j, const Tables& T, uint32_t c, int from, bool* carried) {
	const uint32_t first = c * (uint32_t)kChunkLanes;
	unsigned long long out = c + 1 < j.chunks ? j.carry[from][c + 1] : 0;
	uint32_t decoded = 0;
	if (c > 0 && j.carry[from][c] != j.st[first]) {
		j.st[first] = j.carry[from][c];
		State s = unpack(j.st[first]);
		uint32_t at = first;
		for (int t = 0; t < kChunkLanes; ++t) {
			const LaneView v = lane_view(j, at);
			s = run_subsequence(v.b, v.sg.len, T, j.lay, s, end_position(v.sg.len, v.i, j.subseq_bytes), j.subseq_bytes);
			++decoded;
			if (v.i + 1 == v.sg.lanes) break;
			const uint32_t next = at + 1;
			if (next == first + (uint32_t)kChunkLanes) {
				if (pack(s) != out) { out = pack(s); *carried = true; }
				break;
			}
			at = next;
			if (!store_if_new(&j.st[next], s)) break;
		}
	}
	if (c + 1 < j.chunks) j.carry[1 - from][c + 1] = out;
	return decoded;
}

struct CensusSink {
	uint32_t began = 0;
	DVP_JH_HD void begin(uint32_t, int) { ++began; }
	DVP_JH_HD void symbol(const Step&) {}
	DVP_JH_HD void end(uint32_t) {}
};
// false: the lane does not leave in the next lane's entry state (the synchronisation has not converged), or met rubbish
DVP_JH_HD inline bool census_lane(const Job& j, const Tables& T, uint32_t lane) {
	const LaneView v = lane_view(j, lane);
	const uint32_t end_bit = end_position(v.sg.len, v.i, j.subseq_bytes);
	CensusSink sink;
	State leaves = unpack(j.st[lane]);
	const bool ran = run_blocks(v.b, v.sg.len, T, j.lay, unpack(j.st[lane]), end_bit, j.subseq_bytes, sink, &leaves);
	j.began[lane] = sink.began;
	if (v.i + 1 == v.sg.lanes) return true;   // what follows a segment's last block is padding: nothing to check but the quota (count_lane)
	return ran && pack(leaves) == j.st[lane + 1];
}

struct CountSink {
	const Job& j;
	const LaneView& v;
	uint32_t number, quota;   // the next block's number in the segment
	BlockPlace at = { 0, 0, 0 };
	uint32_t count = 0;
	int diff = 0;
	bool live = false, good = true;
	DVP_JH_HD CountSink(const Job& j_, const LaneView& v_, uint32_t number_, uint32_t quota_) : j(j_), v(v_), number(number_), quota(quota_) {}
	DVP_JH_HD void begin(uint32_t, int blk) {
		live = number < quota;   // (past the quota: the padding, decoded as if it were a block)
		if (live) at = place_of(j.lay, v.seg, number, blk);
		count = 1;
		diff = 0;
	}
	DVP_JH_HD void symbol(const Step& s) {
		if (!live) return;
		if (s.error) good = false;
		if (s.kind == kDc) diff = s.value;
		if (s.kind == kAc && s.value != 0) ++count;
	}
	DVP_JH_HD void end(uint32_t p) {
		if (live) {
			if (j.offsets[at.comp]) j.offsets[at.comp][at.raster_index + 1] = count;
			j.dc[at.comp][at.scan_index] = diff;
			if (number + 1 == quota && !ends_the_segment(v.b, v.sg.len, p)) good = false;
		}
		++number;
	}
};
// false: a corrupt code, or the segment does not hold exactly its quota of MCUs
DVP_JH_HD inline bool count_lane(const Job& j, const Tables& T, uint32_t lane) {
	const LaneView v = lane_view(j, lane);
	const uint32_t number = j.first_block[lane] - j.first_block[v.sg.first_lane], quota = quota_blocks(j.lay, v.seg);
	CountSink sink(j, v, number, quota);
	State leaves;
	const bool ran = run_blocks(v.b, v.sg.len, T, j.lay, unpack(j.st[lane]), end_position(v.sg.len, v.i, j.subseq_bytes), j.subseq_bytes, sink, &leaves);
	if (!sink.good || (!ran && number < quota)) return false;
	if (v.i + 1 == v.sg.lanes && sink.number < quota) return false;   // too few blocks in the segment's bytes
	return true;
}

// the DC prediction of block `index` of component ci (scan order) from the prefix sums: restarted at the segment's first block.
// false: outside the serial scan's limit ("corrupt DC value")
DVP_JH_HD inline bool finish_dc(const Job& j, int ci, uint32_t index) {
	const uint32_t per_segment = (uint32_t)j.lay.interval * (uint32_t)j.lay.c[ci].hv;
	const uint32_t first = index / per_segment * per_segment;
	const long long pred = j.dc_sum[ci][index] - (first ? j.dc_sum[ci][first - 1] : 0);
	j.dc[ci][index] = (int32_t)pred;
	return pred > -kDcLimit && pred < kDcLimit;
}

DVP_JH_HD inline uint32_t make_record(int position, int value) { return ((uint32_t)value << 6) | (uint32_t)position; }   // dvpjdmid::make_record

struct WriteSink {
	const Job& j;
	const LaneView& v;
	const uint8_t* zigzag;
	uint32_t number, quota;
	uint32_t* out = nullptr;
	DVP_JH_HD WriteSink(const Job& j_, const LaneView& v_, const uint8_t* zigzag_, uint32_t number_, uint32_t quota_) : j(j_), v(v_), zigzag(zigzag_), number(number_), quota(quota_) {}
	DVP_JH_HD void begin(uint32_t, int blk) {
		out = nullptr;
		if (number >= quota) return;
		const BlockPlace at = place_of(j.lay, v.seg, number, blk);
		if (!j.offsets[at.comp]) return;   // luma only: decoded, nothing written
		out = j.records[at.comp] + j.offsets[at.comp][at.raster_index];
		*out++ = make_record(0, j.dc[at.comp][at.scan_index]);
	}
	DVP_JH_HD void symbol(const Step& s) {
		if (out && s.kind == kAc && s.value != 0) *out++ = make_record(zigzag[s.k], s.value);
	}
	DVP_JH_HD void end(uint32_t) { ++number; }
};
DVP_JH_HD inline void write_lane(const Job& j, const Tables& T, uint32_t lane) {
	const LaneView v = lane_view(j, lane);
	WriteSink sink(j, v, T.zigzag, j.first_block[lane] - j.first_block[v.sg.first_lane], quota_blocks(j.lay, v.seg));
	State leaves;
	(void)run_blocks(v.b, v.sg.len, T, j.lay, unpack(j.st[lane]), end_position(v.sg.len, v.i, j.subseq_bytes), j.subseq_bytes, sink, &leaves);
}

}   // namespace dvpjh

// ---- the host's half: the pre-scan and the plan of a file (needs dvp_jpeg_dec_mid.hpp before this header) ------------------------
#if defined(DVP_JPEG_DEC_MID_HPP_)
#include <vector>

namespace dvpjh {

struct Plan {
	std::vector<Seg> segs;
	std::vector<uint32_t> lane_seg;
	Tables tables;
	Layout lay;
	const uint8_t* data = nullptr;
	size_t data_bytes = 0;        // the entropy-coded bytes, RSTn markers included, without the marker that ends them
	uint32_t lanes = 0, chunks = 0;
	size_t blocks[3] = { 0, 0, 0 };
	const char* why_not = "";     // when plan() returns false: why the serial scan has to take the file
};

// What Decoder::scan does before its first bit — the checks, the components' block counts, `want` — and one pass over the scan's
// bytes for the segments.  `d` has been parsed with stop_at_scan.  false: the file is one for the serial scan (which will accept it
// or refuse it with its own message); nothing here refuses a file.
inline bool plan(dvpjdmid::Decoder& d, bool luma_only, int subseq_bytes, Plan* out) {
	auto no = [&](const char* why) { out->why_not = why; return false; };
	if (!d.scan_data) return no("no scan");
	const int n = (int)d.comps.size();
	const int mcu_w = 8 * d.hmax, mcu_h = 8 * d.vmax;
	const long long mcus_x = (d.width + mcu_w - 1) / mcu_w, mcus_y = (d.height + mcu_h - 1) / mcu_h;
	if (mcus_x * mcus_y * mcu_w * mcu_h >= 0x80000000LL) return no("too large");   // (block and record numbers stay 32-bit)
	Layout& lay = out->lay;
	lay = Layout();
	lay.comps = n;
	lay.mcus_x = (int)mcus_x;
	lay.total_mcus = (int)(mcus_x * mcus_y);
	lay.interval = d.restart_interval > 0 && d.restart_interval < lay.total_mcus ? d.restart_interval : lay.total_mcus;
	int blk = 0;
	for (int i = 0; i < n; ++i) {
		dvpjdmid::Component& c = d.comps[i];
		if (c.td > 3 || c.ta > 3 || !d.have_qt[c.tq] || !d.dc[c.td].ok || !d.ac[c.ta].ok) return no("tables");
		if (blk + c.h * c.v > kMaxMcuBlocks) return no("more than ten blocks per MCU");
		c.blocks_w = (int)mcus_x * c.h;
		c.blocks_h = (int)mcus_y * c.v;
		c.want = !luma_only || i == 0;
		lay.c[i] = CompLayout{ c.h, c.v, c.h * c.v, c.blocks_w, c.td, c.ta, c.want ? 1 : 0, blk };
		for (int k = 0; k < c.h * c.v; ++k) lay.blk_comp[blk++] = (uint8_t)i;
		out->blocks[i] = (size_t)c.blocks_w * c.blocks_h;
	}
	lay.mcu_blocks = blk;
	if (luma_only && (d.comps[0].h != d.hmax || d.comps[0].v != d.vmax)) return no("sub-sampled luma");
	for (int t = 0; t < 8; ++t) {
		const dvpjdmid::Huff& h = t < 4 ? d.dc[t] : d.ac[t - 4];
		Table& to = out->tables.t[t];
		for (int l = 0; l <= 16; ++l) {   // (a table no DHT gave matches nothing; no component of this scan uses one)
			const bool has = h.ok && l > 0;
			to.mincode[l] = has ? h.mincode[l] : 0;
			to.maxcode[l] = has ? h.maxcode[l] : -1;
			to.valptr[l] = has ? h.valptr[l] : 0;
		}
		for (int k = 0; k < 256; ++k) to.vals[k] = h.vals[k];
	}
	for (int k = 0; k < 64; ++k) out->tables.zigzag[k] = dvpjdmid::zigzag()[k];
	// the segments
	const uint8_t* b = d.scan_data;
	const size_t size = (size_t)(d.scan_end - d.scan_data);
	const size_t expected = (size_t)((lay.total_mcus + lay.interval - 1) / lay.interval);
	out->segs.clear();
	out->lane_seg.clear();
	size_t from = 0, i = 0;
	bool ended = false;
	auto close = [&](size_t to) {
		const size_t len = to - from;
		if (len == 0 || len >= kSegmentBytesMax || from >= 0xFFFFFFFFull) return false;
		const uint32_t lanes = (uint32_t)((len + (size_t)subseq_bytes - 1) / (size_t)subseq_bytes);
		out->segs.push_back(Seg{ (uint32_t)from, (uint32_t)len, (uint32_t)out->lane_seg.size(), lanes });
		out->lane_seg.insert(out->lane_seg.end(), lanes, (uint32_t)(out->segs.size() - 1));
		return true;
	};
	while (i < size) {
		if (b[i] != 0xFF) { ++i; continue; }
		if (i + 1 >= size) return no("no marker ends the scan");
		const int m = b[i + 1];
		if (m == 0) { i += 2; continue; }
		if (m == 0xFF) return no("fill bytes");
		if (m >= 0xD0 && m <= 0xD7) {
			if (out->segs.size() + 1 >= expected) return no("more restart markers than intervals");
			if (!close(i)) return no("an empty or oversized segment");
			from = i = i + 2;
			continue;
		}
		if (!close(i)) return no("an empty or oversized segment");
		ended = true;
		break;
	}
	if (!ended) return no("no marker ends the scan");
	if (out->segs.size() != expected) return no("fewer restart markers than intervals");
	out->data = b;
	out->data_bytes = i;
	out->lanes = (uint32_t)out->lane_seg.size();
	out->chunks = (out->lanes + (uint32_t)kChunkLanes - 1) / (uint32_t)kChunkLanes;
	return true;
}

}   // namespace dvpjh
#endif
#endif
