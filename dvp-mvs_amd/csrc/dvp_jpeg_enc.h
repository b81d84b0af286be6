// dvp_jpeg_enc.h — the device JPEG encoder and preview renderer (dvp_jpeg.hip) as the engine's contexts use them.
#ifndef DVP_JPEG_ENC_H_
#define DVP_JPEG_ENC_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dvp_devmem.hpp"
#include "dvp_jpeg.hpp"

namespace dvpjpeg {

// Device scratch of one image's encode; buffers grow and are kept for the next image of the same or a smaller size.
struct Encoder {
	int W = 0, H = 0, C = 0, R = 0, bpm = 0;
	long long nmcu = 0, nseg = 0;
	Tables tab{};                       // host copy (headers, and the source of the device copy)
	dvpmem::DevBlock d_tab;             // Tables
	dvpmem::DevBlock coef;              // int16_t [nmcu * bpm][64] zig-zag
	dvpmem::DevBlock mask;              // uint64_t [nmcu * bpm]
	dvpmem::DevBlock seglen;            // unsigned [nseg + 1]
	dvpmem::DevBlock segoff;            // unsigned long long [nseg + 1]: exclusive scan, [nseg] = total
	dvpmem::DevBlock out;               // entropy-coded segments with their RST markers
	unsigned long long data_bytes = 0;
	uint8_t header[1024];
	int header_len = 0;
	const char* error = nullptr;
};

// the engine's choice of restart interval, in MCUs
int default_restart(int channels);
// Steps 1-3 on `stream`: coefficients, segment sizes, their scan; the total is copied (asynchronously) to *total_host, which
// must stay valid until the stream reaches it.  pixels: device memory, `pitch` bytes per row, BGR or grey.
int encode_begin(Encoder& e, hipStream_t stream, const uint8_t* pixels, long long pitch, int W, int H, int C, int quality,
                 int restart, unsigned long long* total_host);
// Step 4 once the total is known on the host: grows the output buffer and codes every segment to its offset.
int encode_write(Encoder& e, hipStream_t stream, unsigned long long total);
// header + data + EOI; the bytes a finished encode occupies in a file
inline unsigned long long file_bytes(const Encoder& e) { return (unsigned long long)e.header_len + e.data_bytes + 2; }

// The three preview renderers over L pixels of the context's planes (x, y, z, w per pixel) and weak map; NULL outputs are
// skipped.  BGR, 3 bytes per pixel.
int launch_render(hipStream_t stream, const float* planes, const uint8_t* weak, size_t L, float dmin, float dmax,
                  uint8_t* depth_bgr, uint8_t* normal_bgr, uint8_t* weak_bgr);

}   // namespace dvpjpeg
#endif
