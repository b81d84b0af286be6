// dvp_cloudeval_run.h — the distance stage of dvp_cloudeval.hip for a caller that already has both clouds on the device
// (dvp_cloudprep.hip's dvp_cloud_evaluate_prepared).
#ifndef DVP_CLOUDEVAL_RUN_H_
#define DVP_CLOUDEVAL_RUN_H_

#include "dvp_cloudeval.hpp"

namespace dvpce {

// dvp_cloud_evaluate's definition on two clouds in device memory (packed float triples, num[c] points, not changed), bounds[c] the
// extent and the count of cloud c's points with three finite coordinates.  dev_d2_first (may be NULL): device memory for num[0]
// floats that receives cloud 0's distances (dvp_cloudscan.hip counts from them there).  Non-zero: dvp_cloud_last_error() says why,
// under `who`.
int cloud_run_on_device(const char* who, int device, const float* const dev_xyz[2], const long long num[2], const Bounds bounds[2], const float* tolerances, int num_tol,
                        long long* const within[2], long long* used, float* const d2[2], float* dev_d2_first = nullptr);

}   // namespace dvpce
#endif
