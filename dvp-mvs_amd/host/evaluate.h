// evaluate.h — `apd --evaluate`: a fused cloud scored against a ground-truth cloud (accuracy, completeness, F1 per tolerance) on the
// device (dvp_cloud_evaluate) or, the same text, on the host.  host/ply.cpp, host/evaluate.cpp; csrc/dvp_cloudeval.hpp holds the
// definition, DESIGN.md "Cloud evaluation" what is out of scope.
#ifndef DVP_HOST_EVALUATE_H_
#define DVP_HOST_EVALUATE_H_
#include <string>
#include <vector>

// The vertices of a PLY file as packed x y z floats.  Formats binary_little_endian and ascii; x, y, z float or double (a double is
// rounded to binary32) among any other scalar properties; a fixed-size element before `vertex` is skipped, those after it are
// ignored.  false: *error says what is wrong (binary_big_endian, a list property in or before `vertex`, a short body, a missing x,
// y or z ...).
bool ReadPlyVertices(const std::string& file, std::vector<float>* xyz, std::string* error);

struct EvaluateOptions {
	std::string recon, truth, out;   // out: the report is also written there ("" = stdout only)
	std::vector<float> tolerances = { 0.01f, 0.02f, 0.05f, 0.1f, 0.2f, 0.5f };   // ETH3D's, in metres
	bool on_gpu = true;              // false: csrc/dvp_cloudeval.hpp's serial text on the host
	int device = 0;
};
// the report of two counted clouds: the same bytes whichever flavour made the counts
std::string EvaluateReport(const EvaluateOptions& options, const long long num[2], const long long used[2], const long long* within_recon, const long long* within_truth);
// Reads both files, counts, *report = the text.  false: *error says what stopped it.
bool EvaluateClouds(const EvaluateOptions& options, std::string* report, std::string* error);
#endif
