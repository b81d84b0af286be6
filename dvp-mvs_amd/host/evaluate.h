// evaluate.h — `apd --evaluate`: a fused cloud scored against a ground-truth cloud (accuracy, completeness, F1 per tolerance) on the
// device (dvp_cloud_evaluate) or, the same text, on the host.  host/ply.cpp, host/evaluate.cpp; csrc/dvp_cloudeval.hpp holds the
// definition, DESIGN.md "Cloud evaluation" what is out of scope.
#ifndef DVP_HOST_EVALUATE_H_
#define DVP_HOST_EVALUATE_H_
#include <string>
#include <vector>

#include "../csrc/dvp_cloudicp.hpp"
#include "../csrc/dvp_cloudprep.hpp"

// The vertices of a PLY file as packed x y z floats.  Formats binary_little_endian and ascii; x, y, z float or double (a double is
// rounded to binary32) among any other scalar properties; a fixed-size element before `vertex` is skipped, those after it are
// ignored.  false: *error says what is wrong (binary_big_endian, a list property in or before `vertex`, a short body, a missing x,
// y or z ...).
bool ReadPlyVertices(const std::string& file, std::vector<float>* xyz, std::string* error);

struct EvaluateOptions {
	std::string recon, truth, out;   // out: the report is also written there ("" = stdout only)
	std::vector<float> tolerances = { 0.01f, 0.02f, 0.05f, 0.1f, 0.2f, 0.5f };   // ETH3D's, in metres
	bool on_gpu = true;              // false: csrc/dvp_cloudeval.hpp's and csrc/dvp_cloudprep.hpp's serial text on the host
	int device = 0;
	// the preparation of the clouds before they are measured (csrc/dvp_cloudprep.hpp); with none of the three the clouds are taken as read
	std::string transform_file;      // --transform: 16 numbers, applied to the reconstruction only
	std::string crop_file;           // --crop: a SelectionPolygonVolume JSON, applied to both clouds after the transform
	double voxel = 0.0;              // --voxel-size: both clouds, each on its own grid
	std::string save_prepared;       // --save-prepared PREFIX: <PREFIX>recon.ply and <PREFIX>truth.ply
	// the alignment refined before the clouds are measured (csrc/dvp_cloudicp.hpp): the evaluation then takes the refined matrix as if
	// --transform had given it
	std::vector<dvpci::Stage> refine;   // --refine-alignment V:D:N[,V:D:N...]: ICP stages (voxel, distance, iterations), in order
	std::string save_transform;         // --save-transform FILE: the refined matrix, a file --transform reads
	// the ground truth as laser scans (csrc/dvp_cloudscan.hpp): the truth cloud is the scans' points brought into the scene, and the
	// accuracy is the observed-space one - a reconstructed point away from the truth counts only where a scanner looked through it
	std::string truth_scans;            // --against-scans FILE.mlp, in place of --against: ETH3D's scan_alignment.mlp
	int cube_size = 1024;               // --cube-size R: the scans' cube maps hold 6 R R texels each
	bool prepares() const { return !transform_file.empty() || !crop_file.empty() || voxel != 0.0 || !refine.empty(); }
};
// V:D:N[,V:D:N...] -> stages; false: *error says what is wrong (another shape, a word that is no number, more than 8 stages; the
// numbers' ranges are checked where the stages run)
bool ParseRefineStages(const std::string& list, std::vector<dvpci::Stage>* stages, std::string* error);
// 16 numbers as %.17g, four per line: a file ReadTransformFile takes and reads back to the same bits
bool WriteTransformFile(const std::string& file, const double m[16], std::string* error);
// the report's lines about a refinement: one per stage, then the matrix's four rows
std::string AlignmentReport(const std::vector<dvpci::LogRecord>& log, const double m[16]);
// 16 numbers separated by whitespace; false: *error says what is wrong (another count, a word that is no number, a non-finite entry, a last row other than 0 0 0 1)
bool ReadTransformFile(const std::string& file, double m[16], std::string* error);
// Open3D's SelectionPolygonVolume JSON -> prep's crop; false: *error says what is wrong (malformed JSON, a missing field, fewer than 3 or more than 256 vertices ...)
bool ReadCropFile(const std::string& file, dvpcp::Prep* prep, std::string* error);
// One scan of a MeshLab project: the file name as the project writes it, the path it stands for (relative names are taken from the
// project's folder) and the 4 x 4 row-major matrix of its <MLMatrix44>
struct ScanEntry {
	std::string name, path;
	double m[16];
};
// The <MLMesh filename=...> elements of a MeshLab project (.mlp) with their <MLMatrix44>; attributes in any order, single or double
// quotes, whitespace anywhere between the numbers, every other element and attribute ignored.  false: *error says what is wrong (no
// MLMesh element, one without a filename or without a matrix, another count than 16 numbers, a word that is no number, a non-finite
// entry, a last row other than 0 0 0 1, more than 64 scans)
bool ReadScanProject(const std::string& file, std::vector<ScanEntry>* scans, std::string* error);
// binary_little_endian, float x y z only: a file ReadPlyVertices takes
bool WritePlyVertices(const std::string& file, const std::vector<float>& xyz, std::string* error);
// the report of two counted clouds: the same bytes whichever flavour made the counts.  counts (2 x 4: finite, after the transform,
// inside the crop, output points; NULL without a preparation) adds the two `prepared` lines, and `used` then counts prepared points.
// scan_lines / free_space (--against-scans only): the lines about the scans that follow `ground_truth`, and the counts that make the
// accuracy column the observed-space one, accurate / (accurate + free_space), and add the table of the three classes.
std::string EvaluateReport(const EvaluateOptions& options, const long long num[2], const long long used[2], const long long* within_recon, const long long* within_truth,
                           const long long* counts = nullptr, const std::string& scan_lines = "", const long long* free_space = nullptr);
// Reads both files, counts, *report = the text.  false: *error says what stopped it.
bool EvaluateClouds(const EvaluateOptions& options, std::string* report, std::string* error);
#endif
