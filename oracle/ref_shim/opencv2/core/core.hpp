// REFERENCE PIN — TEST INFRASTRUCTURE ONLY.
// Stand-in for OpenCV: the names APD.h / main.h mention in host declarations (never called by the
// device text) and the two macros the device text does use.
#ifndef DVP_REF_SHIM_OPENCV_CORE_HPP_
#define DVP_REF_SHIM_OPENCV_CORE_HPP_
typedef unsigned char uchar;
// opencv2/core/cvdef.h (oracle contract list, ora_common.h)
#ifndef MIN
#define MIN(a, b) ((a) > (b) ? (b) : (a))
#endif
#ifndef MAX
#define MAX(a, b) ((a) < (b) ? (b) : (a))
#endif
namespace cv {
struct Mat {};
template <class T> struct Mat_ {};
struct Vec3f {};
struct Vec3b {};
struct Point { int x = 0, y = 0; };
struct Size2i { int width = 0, height = 0; };
}  // namespace cv
#endif
