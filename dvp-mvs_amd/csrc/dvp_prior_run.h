// dvp_prior_run.h — the monocular-depth plane prior on the device (dvp_prior.hip) as the engine's contexts use it.
#ifndef DVP_PRIOR_RUN_H_
#define DVP_PRIOR_RUN_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/dvp_mvs.h"
#include "dvp_devmem.hpp"
#include "dvp_prior.hpp"

namespace dvpprior {

// Device scratch of a context, one allocation that grows on demand and is kept for the next view: the dep map, the owner map, the
// rate map (4 bytes per dep-map pixel each), the working-size depth (4 bytes per context pixel), the triangle list, the row
// offsets and the counter sequences (one float per sweep row).
struct Scratch {
	dvpmem::DevBlock pool;
	// the pool's parts for the geometry of the last run
	float* raw = nullptr; int32_t* owner = nullptr; float* rate = nullptr; float* depth = nullptr;
	Tri* tris = nullptr; unsigned* row_off = nullptr; float* seq = nullptr;
	int cols = 0, rows = 0, W = 0, H = 0;
	bool ran = false;                       // the maps above are those of a finished run with status 0
	std::vector<Tri> tris_host;
	std::vector<unsigned> row_off_host;     // [triangles + 1] exclusive prefix sum of the triangles' row counts
	double ms[3] = { 0, 0, 0 };             // the host part (points, triangulation, row counts), the uploads, the kernels
	long long triangles = 0, sweep_rows = 0;
};
// The whole prior on `stream`: the host part (dvp_prior_mid.hpp), the uploads, five launches whatever the inputs hold, one wait at
// the end.  cam: the context's reference camera ON THE DEVICE (intrinsics at the working size W x H); planes: W * H float4 on the
// device.  *status = 1 (planes untouched, nothing launched): an empty map or no usable point.  Non-zero: *error says why.
int run(hipStream_t stream, Scratch& s, const float* dep_raw, int cols, int rows, const float* xy, const float* xyz, int num_points, const DvpCamera* file_camera,
        const DvpCamera* cam, int W, int H, void* planes, int* status, const char** error);
// after a run with status 0: DVP_PRIOR_STAGE_* to the host
int stage(hipStream_t stream, Scratch& s, int which, void* dst, const char** error);

}   // namespace dvpprior
#endif
