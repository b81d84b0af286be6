// evaluate.cpp — `apd --evaluate recon.ply --against truth.ply` (evaluate.h): both clouds read, the two directions counted on the
// device (dvp_cloud_evaluate) or by the same text on the host (csrc/dvp_cloudeval.hpp: the double loop up to 2^24 pairs, the grid
// walked serially above), and the report, whose figures come from the integer counts alone.
#include "evaluate.h"

#include <cstdio>
#include <fstream>
#include <new>

#include "../../include/dvp_mvs.h"
#include "../csrc/dvp_cloudeval.hpp"

std::string EvaluateReport(const EvaluateOptions& o, const long long num[2], const long long used[2], const long long* within_recon, const long long* within_truth) {
	char text[256];
	std::string report = "reconstruction " + o.recon + " " + std::to_string(used[0]) + " points (" + std::to_string(num[0] - used[0]) + " skipped)\n" +
	                     "ground_truth " + o.truth + " " + std::to_string(used[1]) + " points (" + std::to_string(num[1] - used[1]) + " skipped)\n" +
	                     "tolerance accuracy completeness f1\n";
	for (size_t k = 0; k < o.tolerances.size(); ++k) {
		const double a = used[0] ? (double)within_recon[k] / (double)used[0] : 0.0, c = used[1] ? (double)within_truth[k] / (double)used[1] : 0.0;
		const double f = a + c == 0.0 ? 0.0 : 2.0 * a * c / (a + c);
		snprintf(text, sizeof text, "%.9g %.6f %.6f %.6f\n", (double)o.tolerances[k], 100.0 * a, 100.0 * c, 100.0 * f);
		report += text;
	}
	return report;
}

static bool EvaluateCloudsOrThrow(const EvaluateOptions& o, std::string* report, std::string* error);

bool EvaluateClouds(const EvaluateOptions& o, std::string* report, std::string* error) {
	try {
		return EvaluateCloudsOrThrow(o, report, error);
	} catch (const std::bad_alloc&) {   // the clouds, or the host flavour's table, do not fit the host's memory
		*error = "out of host memory";
		return false;
	}
}

static bool EvaluateCloudsOrThrow(const EvaluateOptions& o, std::string* report, std::string* error) {
	std::vector<float> recon, truth;
	if (!ReadPlyVertices(o.recon, &recon, error) || !ReadPlyVertices(o.truth, &truth, error)) return false;
	const long long num[2] = { (long long)(recon.size() / 3), (long long)(truth.size() / 3) };
	const int K = (int)o.tolerances.size();
	long long within_recon[dvpce::kMaxTolerances] = {}, within_truth[dvpce::kMaxTolerances] = {}, used[2] = { 0, 0 };
	if (o.on_gpu) {
		if (dvp_cloud_evaluate(o.device, recon.data(), num[0], truth.data(), num[1], o.tolerances.data(), K, within_recon, within_truth, used, nullptr, nullptr) != 0) {
			*error = dvp_cloud_last_error();
			return false;
		}
	} else {
		const std::string what = K > dvpce::kMaxTolerances ? "at most 8 tolerances" :
		                         dvpce::serial_evaluate(recon.data(), num[0], truth.data(), num[1], o.tolerances.data(), K, within_recon, within_truth, used, nullptr, nullptr);
		if (!what.empty()) { *error = what; return false; }
	}
	*report = EvaluateReport(o, num, used, within_recon, within_truth);
	if (!o.out.empty()) {
		std::ofstream out(o.out, std::ios::binary);
		out << *report;
		if (!out.good()) { *error = "cannot write " + o.out; return false; }
	}
	return true;
}
