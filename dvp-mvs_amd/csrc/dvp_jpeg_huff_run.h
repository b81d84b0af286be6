// dvp_jpeg_huff_run.h — what dvp_jpeg_dec.hip calls of dvp_jpeg_huff.hip: the Huffman scan of one planned file on the device.
#ifndef DVP_JPEG_HUFF_RUN_H_
#define DVP_JPEG_HUFF_RUN_H_

#include <hip/hip_runtime.h>

#include "dvp_devmem.hpp"
#include "dvp_jpeg_dec_mid.hpp"
#include "dvp_jpeg_huff.hpp"

namespace dvpjh {

// the records of a scan in device memory, in the format of dvp_jpeg_dec_mid.hpp; NULL / 0 for a component that is not wanted
struct DeviceScan {
	const uint32_t* offsets[3] = { nullptr, nullptr, nullptr };
	const uint32_t* records[3] = { nullptr, nullptr, nullptr };
	size_t offset_words[3] = { 0, 0, 0 }, record_words[3] = { 0, 0, 0 };
};

enum { kPathHost = 0, kPathDevice = 1, kPathFellBack = 2 };
enum { kMsPrescan = 0, kMsUpload, kMsSync, kMsCount, kMsScans, kMsWrite, kMsReconstruct, kMsPhases };
struct ScanStats {
	long long path = kPathHost, segments = 0, subsequences = 0, chunks = 0, longest = 0, rounds = 0, uploaded = 0, decodes = 0;
	double ms[kMsPhases] = { 0, 0, 0, 0, 0, 0, 0 };   // filled only by a serialised run (DVP_JPEG_ENTROPY_SERIAL=1: a wait after every phase)
};

// Runs the planned scan on `st`: uploads the entropy-coded bytes into `work`, leaves offsets there and the records in `recs`.
// 0: done: *out is complete once the work queued on `st` has run (the write pass is not waited for).  1: the serial scan has to take the file — the fall-back flag, the
// round cap (DVP_TEST_JPEG_SYNC_CAP lowers it) or a refused allocation; *why says which.  Nothing is left half-used either way.
int scan_on_device(const Plan& plan, int subseq_bytes, hipStream_t st, dvpmem::DevBlock& work, dvpmem::DevBlock& recs, DeviceScan* out, ScanStats* stats, const char** why);

int subseq_bytes_in_use();   // kSubseqBytes, or DVP_JPEG_SUBSEQ_BYTES = 64 | 128 | 256 | 512 (for measuring)
bool serialised_run();       // DVP_JPEG_ENTROPY_SERIAL=1

}   // namespace dvpjh
#endif
