// dvp_cloudprep_run.h — the preparation of dvp_cloudprep.hip for a caller whose raw cloud is in device memory already and who keeps
// the prepared cloud there (dvp_cloudicp.hip's stages).
#ifndef DVP_CLOUDPREP_RUN_H_
#define DVP_CLOUDPREP_RUN_H_

#include <hip/hip_runtime.h>

#include "dvp_cloudprep.hpp"
#include "dvp_devmem.hpp"

struct dvp_cloud_prep;

namespace dvpcp {

// the C ABI's description in its parser-independent form, checked as dvp_cloud_prepare checks it; "" or what is wrong
std::string prep_of_abi(const dvp_cloud_prep* c, Prep* prep);

// a prepared cloud in device memory: `num` packed float triples at the start of `out`; bounds: their extent and finite count
struct ResidentCloud {
	dvpmem::DevBlock out;
	long long num = 0, counts[4] = { 0, 0, 0, 0 };   // counts: finite, after the transform, inside the crop, output points
	dvpce::Bounds bounds;
	const float* xyz() const { return out.as<float>(); }
};

// dvp_cloud_prepare's definition on `num` points at dev_xyz (device memory, not changed); `prep` has passed check_prep.  The work
// is queued on `st` and waited for.  "" or the error.
std::string prepare_resident(hipStream_t st, const float* dev_xyz, long long num, const Prep& prep, ResidentCloud* res);

}   // namespace dvpcp
#endif
