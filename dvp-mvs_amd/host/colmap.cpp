// colmap.cpp — `apd --convert-from <colmap folder> <save folder>`: the reference's colmap2mvsnet.py without OpenCV and numpy.
//   readers      cameras / images / points3D as .txt or .bin (colmap2mvsnet.py:60-237); the images renumbered 0 .. n-1 by COLMAP id
//   cameras      intrinsics from the script's parameter-name table, extrinsics with qvec2rotmat's operation order, the depth range
//                from the sorted camera-space z of the view's points (colmap2mvsnet.py:338-402)
//   pair.txt     the view-selection scores (csrc/dvp_pairs.hpp: dvp_view_scores on the device, or the same text here), the rows in
//                the script's layout
//   images/      every input decoded (baseline JPEG, binary PGM / PPM), padded and resampled (csrc/dvp_pairs.hpp: dvp_convert_image
//                or the same text here), encoded by dvp_jpeg_encode at quality 95
//   sfm/         the project's own file, which nothing in the reference writes: one line per observation with a point, what
//                host/prior.cpp reads
//   --undistort on   the project's own stage too (csrc/dvp_undistort.hpp): every decoded picture is resampled into the pinhole camera
//                the cams already describe - dvp_undistort_image or the same text here - before it is padded, and sfm/ holds the
//                points' pinhole projections in place of the observations made in the distorted picture
// Plain C++: the device is reached through the C ABI only.
#include "colmap.h"

#include <array>
#include <cerrno>
#include <map>

#include "../csrc/dvp_pairs.hpp"
#include "../csrc/dvp_undistort.hpp"
#include "APD.h"

namespace {

struct ModelKind { int id; const char* name; int num_params; bool single_f; };
// CAMERA_MODELS (colmap2mvsnet.py:33-45) with the parameter-name table (322-334): `f` stands for fx and fy, then cx, cy
const ModelKind kModels[11] = {
	{ 0, "SIMPLE_PINHOLE", 3, true }, { 1, "PINHOLE", 4, false }, { 2, "SIMPLE_RADIAL", 4, true }, { 3, "RADIAL", 5, true }, { 4, "OPENCV", 8, false }, { 5, "OPENCV_FISHEYE", 8, false },
	{ 6, "FULL_OPENCV", 12, false }, { 7, "FOV", 5, false }, { 8, "SIMPLE_RADIAL_FISHEYE", 4, true }, { 9, "RADIAL_FISHEYE", 5, true }, { 10, "THIN_PRISM_FISHEYE", 12, false },
};
const ModelKind* kind_by_name(const std::string& name) {
	for (const ModelKind& k : kModels)
		if (name == k.name) return &k;
	return nullptr;
}
const ModelKind* kind_by_id(int id) { return id >= 0 && id < 11 ? &kModels[id] : nullptr; }

std::vector<std::string> split(const std::string& line) {
	std::vector<std::string> out;
	std::istringstream in(line);
	std::string s;
	while (in >> s) out.push_back(s);
	return out;
}
bool to_int(const std::string& s, long long* v) {
	errno = 0;
	char* end = nullptr;
	*v = strtoll(s.c_str(), &end, 10);
	return !s.empty() && *end == 0 && errno == 0;
}
bool to_double(const std::string& s, double* v) {
	char* end = nullptr;
	*v = strtod(s.c_str(), &end);
	return !s.empty() && *end == 0;
}

// a text file line by line with the reference's rule for record lines: stripped, not empty, not a comment
struct TextFile {
	std::ifstream in;
	std::string name;
	long long line_no = 0;
	bool open(const path& p) { name = p.filename().string(); in.open(p); return (bool)in; }
	bool raw(std::string* line) { if (!std::getline(in, *line)) return false; ++line_no; return true; }
	bool record(std::vector<std::string>* elems) {
		std::string line;
		while (raw(&line)) {
			*elems = split(line);
			if (!elems->empty() && (*elems)[0][0] != '#') return true;
		}
		return false;
	}
	std::string here() const { return name + ":" + std::to_string(line_no); }
};

struct BinFile {
	std::ifstream in;
	std::string name;
	long long size = 0;
	bool open(const path& p) {
		name = p.filename().string();
		in.open(p, std::ios::binary);
		std::error_code ec;
		size = (long long)std::filesystem::file_size(p, ec);
		return (bool)in && !ec;
	}
	template <class T>
	bool get(T* v) { in.read(reinterpret_cast<char*>(v), sizeof(T)); return in.gcount() == (std::streamsize)sizeof(T); }   // (little-endian hosts, as COLMAP writes)
};

bool fail(std::string* error, const std::string& what) { *error = what; return false; }

bool read_cameras_text(const path& p, ColmapModel* m, std::string* error) {
	TextFile f;
	if (!f.open(p)) return fail(error, "cannot open " + p.string());
	std::vector<std::string> e;
	while (f.record(&e)) {
		ColmapCamera c;
		long long id = 0;
		if (e.size() < 4) return fail(error, f.here() + ": a short line (camera id, model, width, height, parameters)");
		if (!to_int(e[0], &id) || !to_int(e[2], &c.width) || !to_int(e[3], &c.height)) return fail(error, f.here() + ": the id, width and height must be integers");
		c.id = (int)id;
		c.model = e[1];
		const ModelKind* k = kind_by_name(c.model);
		if (!k) return fail(error, f.here() + ": unknown camera model " + c.model);
		if ((int)e.size() - 4 < k->num_params) return fail(error, f.here() + ": a short line (" + c.model + " has " + std::to_string(k->num_params) + " parameters)");
		for (size_t i = 4; i < e.size(); ++i) {
			double v = 0;
			if (!to_double(e[i], &v)) return fail(error, f.here() + ": '" + e[i] + "' is not a number");
			c.params.push_back(v);
		}
		m->cameras.push_back(c);
	}
	return true;
}

bool read_cameras_binary(const path& p, ColmapModel* m, std::string* error) {
	BinFile f;
	if (!f.open(p)) return fail(error, "cannot open " + p.string());
	uint64_t n = 0;
	if (!f.get(&n)) return fail(error, f.name + ": truncated (the camera count)");
	for (uint64_t r = 0; r < n; ++r) {
		const std::string here = f.name + ": record " + std::to_string(r);
		int32_t id = 0, model = 0;
		uint64_t w = 0, h = 0;
		if (!f.get(&id) || !f.get(&model) || !f.get(&w) || !f.get(&h)) return fail(error, here + ": truncated");
		const ModelKind* k = kind_by_id(model);
		if (!k) return fail(error, here + ": unknown camera model " + std::to_string(model));
		ColmapCamera c;
		c.id = id; c.model = k->name; c.width = (long long)w; c.height = (long long)h;
		c.params.resize((size_t)k->num_params);
		for (double& v : c.params)
			if (!f.get(&v)) return fail(error, here + ": truncated");
		m->cameras.push_back(c);
	}
	return true;
}

bool read_images_text(const path& p, ColmapModel* m, std::string* error) {
	TextFile f;
	if (!f.open(p)) return fail(error, "cannot open " + p.string());
	std::vector<std::string> e;
	while (f.record(&e)) {
		ColmapImage im;
		im.where = f.here();
		long long id = 0, cam = 0;
		if (e.size() < 10) return fail(error, f.here() + ": a short line (image id, 4 quaternion and 3 translation entries, camera id, name)");
		bool ok = to_int(e[0], &id) && to_int(e[8], &cam);
		for (int i = 0; i < 4; ++i) ok = ok && to_double(e[1 + i], &im.q[i]);
		for (int i = 0; i < 3; ++i) ok = ok && to_double(e[5 + i], &im.t[i]);
		if (!ok) return fail(error, f.here() + ": a malformed number");
		im.id = (int)id; im.camera_id = (int)cam; im.name = e[9];
		// the line after it holds the observations, whatever it looks like (colmap2mvsnet.py:137)
		std::string line;
		if (f.raw(&line)) {
			const std::vector<std::string> o = split(line);
			if (o.size() % 3 != 0) return fail(error, f.here() + ": a short line (x, y and a point id per observation)");
			for (size_t i = 0; i < o.size(); i += 3) {
				double x = 0, y = 0;
				long long pid = 0;
				if (!to_double(o[i], &x) || !to_double(o[i + 1], &y) || !to_int(o[i + 2], &pid)) return fail(error, f.here() + ": a malformed observation");
				im.xy.push_back(x); im.xy.push_back(y);
				im.point_ids.push_back(pid);
			}
		}
		m->images.push_back(std::move(im));
	}
	return true;
}

bool read_images_binary(const path& p, ColmapModel* m, std::string* error) {
	BinFile f;
	if (!f.open(p)) return fail(error, "cannot open " + p.string());
	uint64_t n = 0;
	if (!f.get(&n)) return fail(error, f.name + ": truncated (the image count)");
	for (uint64_t r = 0; r < n; ++r) {
		const std::string here = f.name + ": record " + std::to_string(r);
		ColmapImage im;
		im.where = here;
		int32_t id = 0, cam = 0;
		bool ok = f.get(&id);
		for (int i = 0; i < 4; ++i) ok = ok && f.get(&im.q[i]);
		for (int i = 0; i < 3; ++i) ok = ok && f.get(&im.t[i]);
		ok = ok && f.get(&cam);
		if (!ok) return fail(error, here + ": truncated");
		im.id = id; im.camera_id = cam;
		for (;;) {
			char c = 0;
			if (!f.get(&c)) return fail(error, here + ": truncated (the name)");
			if (c == 0) break;
			im.name.push_back(c);
		}
		uint64_t k = 0;
		if (!f.get(&k)) return fail(error, here + ": truncated");
		if (k > 0x7fffffffULL) return fail(error, here + ": more than 2^31 - 1 observations");
		for (uint64_t i = 0; i < k; ++i) {
			double x = 0, y = 0;
			int64_t pid = 0;
			if (!f.get(&x) || !f.get(&y) || !f.get(&pid)) return fail(error, here + ": truncated (observation " + std::to_string(i) + " of " + std::to_string(k) + ")");
			im.xy.push_back(x); im.xy.push_back(y);
			im.point_ids.push_back((long long)pid);
		}
		m->images.push_back(std::move(im));
	}
	return true;
}

bool read_points_text(const path& p, ColmapModel* m, std::string* error) {
	TextFile f;
	if (!f.open(p)) return fail(error, "cannot open " + p.string());
	std::vector<std::string> e;
	while (f.record(&e)) {
		ColmapPoint pt;
		if (e.size() < 8) return fail(error, f.here() + ": a short line (point id, x, y, z, r, g, b, error, track)");
		long long c[3] = { 0, 0, 0 };
		double err = 0;
		bool ok = to_int(e[0], &pt.id) && to_double(e[7], &err);
		for (int i = 0; i < 3; ++i) ok = ok && to_double(e[1 + i], &pt.xyz[i]) && to_int(e[4 + i], &c[i]);
		if (!ok) return fail(error, f.here() + ": a malformed number");
		for (int i = 0; i < 3; ++i) pt.rgb[i] = (int)c[i];
		m->points.push_back(pt);
	}
	return true;
}

bool read_points_binary(const path& p, ColmapModel* m, std::string* error) {
	BinFile f;
	if (!f.open(p)) return fail(error, "cannot open " + p.string());
	uint64_t n = 0;
	if (!f.get(&n)) return fail(error, f.name + ": truncated (the point count)");
	for (uint64_t r = 0; r < n; ++r) {
		const std::string here = f.name + ": record " + std::to_string(r);
		ColmapPoint pt;
		uint64_t id = 0, track = 0;
		uint8_t c[3] = { 0, 0, 0 };
		double err = 0;
		bool ok = f.get(&id);
		for (int i = 0; i < 3; ++i) ok = ok && f.get(&pt.xyz[i]);
		for (int i = 0; i < 3; ++i) ok = ok && f.get(&c[i]);
		ok = ok && f.get(&err) && f.get(&track);
		if (!ok) return fail(error, here + ": truncated");
		pt.id = (long long)id;
		for (int i = 0; i < 3; ++i) pt.rgb[i] = c[i];
		// the track itself is skipped: the images' own lists are used instead
		if (track > (uint64_t)f.size / 8) return fail(error, here + ": truncated (the track)");
		f.in.seekg((std::streamoff)(8 * track), std::ios::cur);
		if (!f.in || (long long)f.in.tellg() > f.size) return fail(error, here + ": truncated (the track)");
		m->points.push_back(pt);
	}
	return true;
}

}   // namespace

bool ReadColmapModel(const path& dir, const std::string& ext, ColmapModel* m, std::string* error) {
	*m = ColmapModel();
	if (ext != ".txt" && ext != ".bin") return fail(error, "the model format must be .txt or .bin");
	const bool text = ext == ".txt";
	if (!(text ? read_cameras_text(dir / "cameras.txt", m, error) : read_cameras_binary(dir / "cameras.bin", m, error))) return false;
	if (!(text ? read_images_text(dir / "images.txt", m, error) : read_images_binary(dir / "images.bin", m, error))) return false;
	if (!(text ? read_points_text(dir / "points3D.txt", m, error) : read_points_binary(dir / "points3D.bin", m, error))) return false;
	std::stable_sort(m->images.begin(), m->images.end(), [](const ColmapImage& a, const ColmapImage& b) { return a.id < b.id; });
	for (size_t i = 1; i < m->images.size(); ++i)
		if (m->images[i].id == m->images[i - 1].id) return fail(error, m->images[i].where + ": image id " + std::to_string(m->images[i].id) + " occurs twice");
	if (m->images.empty()) return fail(error, std::string("images") + ext + ": the model has no images");
	return true;
}

std::string PyFloatStr(double v) {
	if (std::isnan(v)) return "nan";
	if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
	char buf[48];
	for (int prec = 0; prec < 17; ++prec) {   // 17 significant digits always read back
		snprintf(buf, sizeof(buf), "%.*e", prec, v);
		if (strtod(buf, nullptr) == v) break;
	}
	std::string s = buf, sign, digits;
	if (s[0] == '-') { sign = "-"; s.erase(0, 1); }
	const size_t e = s.find('e');
	for (size_t i = 0; i < e; ++i)
		if (s[i] != '.') digits.push_back(s[i]);
	const int decpt = atoi(s.c_str() + e + 1) + 1;
	const int nd = (int)digits.size();
	if (decpt <= -4 || decpt > 16) {
		std::string out = sign + digits.substr(0, 1);
		if (nd > 1) out += "." + digits.substr(1);
		const int x = decpt - 1;
		char tail[16];
		snprintf(tail, sizeof(tail), "e%c%02d", x < 0 ? '-' : '+', x < 0 ? -x : x);
		return out + tail;
	}
	if (decpt <= 0) return sign + "0." + std::string((size_t)-decpt, '0') + digits;
	if (decpt >= nd) return sign + digits + std::string((size_t)(decpt - nd), '0') + ".0";
	return sign + digits.substr(0, (size_t)decpt) + "." + digits.substr((size_t)decpt);
}

std::string PairText(const uint32_t* score, int n) {
	std::ostringstream out;
	out << n << "\n";
	const int listed = std::min(20, n - 1);
	std::vector<int> order((size_t)n);
	for (int i = 0; i < n; ++i) {
		const uint32_t* row = score + (size_t)i * n;
		for (int k = 0; k < n; ++k) order[(size_t)k] = k;
		// a stable ascending sort read backwards (np.argsort(score[i])[::-1]): descending score, ties by descending index
		std::sort(order.begin(), order.end(), [row](int a, int b) { return row[a] != row[b] ? row[a] > row[b] : a > b; });
		out << i << "\n" << listed << " ";
		for (int k = 0; k < listed; ++k) out << order[(size_t)k] << " " << row[order[(size_t)k]] << " ";
		out << "\n";
	}
	return out.str();
}

bool ConvertCameras(const ColmapModel& model, const ConvertOptions& opt, ConvertedCameras* out, std::string* error) {
	const size_t n = model.images.size();
	const double F = opt.scale_factor;
	std::map<int, std::array<double, 9>> K;
	for (const ColmapCamera& c : model.cameras) {
		const ModelKind* k = kind_by_name(c.model);
		if (!k || (int)c.params.size() < k->num_params) return fail(error, "camera " + std::to_string(c.id) + ": unknown model or too few parameters");
		const double fx = c.params[0], fy = k->single_f ? c.params[0] : c.params[1], cx = c.params[k->single_f ? 1 : 2], cy = c.params[k->single_f ? 2 : 3];
		K[c.id] = { fx / F, 0, cx / F, 0, fy / F, cy / F, 0, 0, 1 };
	}
	std::map<long long, size_t> point_at;
	for (size_t k = 0; k < model.points.size(); ++k) point_at[model.points[k].id] = k;
	out->extrinsic.assign(16 * n, 0);
	out->intrinsic.assign(9 * n, 0);
	out->depth.assign(4 * n, 0);
	out->centres.assign(3 * n, 0);
	for (size_t i = 0; i < n; ++i) {
		const ColmapImage& im = model.images[i];
		const auto k = K.find(im.camera_id);
		if (k == K.end()) return fail(error, im.where + ": image " + im.name + " names camera " + std::to_string(im.camera_id) + ", which is not in the model");
		std::copy(k->second.begin(), k->second.end(), out->intrinsic.begin() + 9 * i);
		// qvec2rotmat (colmap2mvsnet.py:252-262), operator by operator
		const double* q = im.q;
		double* e = &out->extrinsic[16 * i];
		e[0] = 1 - 2 * (q[2] * q[2]) - 2 * (q[3] * q[3]);
		e[1] = 2 * q[1] * q[2] - 2 * q[0] * q[3];
		e[2] = 2 * q[3] * q[1] + 2 * q[0] * q[2];
		e[4] = 2 * q[1] * q[2] + 2 * q[0] * q[3];
		e[5] = 1 - 2 * (q[1] * q[1]) - 2 * (q[3] * q[3]);
		e[6] = 2 * q[2] * q[3] - 2 * q[0] * q[1];
		e[8] = 2 * q[3] * q[1] - 2 * q[0] * q[2];
		e[9] = 2 * q[2] * q[3] + 2 * q[0] * q[1];
		e[10] = 1 - 2 * (q[1] * q[1]) - 2 * (q[2] * q[2]);
		e[3] = im.t[0]; e[7] = im.t[1]; e[11] = im.t[2];
		e[15] = 1;
		// the camera centre -R^T t (colmap2mvsnet.py:285)
		for (int c = 0; c < 3; ++c) out->centres[3 * i + c] = -(e[c] * e[3] + e[4 + c] * e[7] + e[8 + c] * e[11]);
		// depth range (colmap2mvsnet.py:369-401)
		std::vector<double> zs;
		for (size_t o = 0; o < im.point_ids.size(); ++o) {
			if (im.point_ids[o] == -1) continue;
			const auto at = point_at.find(im.point_ids[o]);
			if (at == point_at.end()) return fail(error, im.where + ": observation " + std::to_string(o) + " of image " + im.name + " names point " + std::to_string(im.point_ids[o]) + ", which is not in points3D");
			const double* p = model.points[at->second].xyz;
			zs.push_back(e[8] * p[0] + e[9] * p[1] + e[10] * p[2] + e[11] * 1.0);
		}
		double depth_min = 0, depth_max = 0;
		if (!zs.empty()) {
			std::sort(zs.begin(), zs.end());
			depth_min = zs[(size_t)(int)((double)zs.size() * .01)] * 0.75;
			depth_max = zs[(size_t)(int)((double)zs.size() * .99)] * 1.25;
		}
		double depth_num = opt.max_d;
		if (opt.max_d == 0) {
			// the inverse-depth rule: the pixel next to the principal point, both at depth_min, taken to the world and measured
			const double* Ki = k->second.data();
			const double a[3] = { 0, 0, depth_min }, b[3] = { (1.0 / Ki[0]) * depth_min, 0, depth_min };   // inv(K) p1 and inv(K) p2, times depth_min
			const double R[9] = { e[0], e[1], e[2], e[4], e[5], e[6], e[8], e[9], e[10] };
			const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
			const double inv[9] = { (R[4] * R[8] - R[5] * R[7]) / det, (R[2] * R[7] - R[1] * R[8]) / det, (R[1] * R[5] - R[2] * R[4]) / det,
				                    (R[5] * R[6] - R[3] * R[8]) / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[2] * R[3] - R[0] * R[5]) / det,
				                    (R[3] * R[7] - R[4] * R[6]) / det, (R[1] * R[6] - R[0] * R[7]) / det, (R[0] * R[4] - R[1] * R[3]) / det };
			double d2 = 0;
			for (int r = 0; r < 3; ++r) {
				double pa = 0, pb = 0;
				for (int c = 0; c < 3; ++c) { pa += inv[3 * r + c] * (a[c] - im.t[c]); pb += inv[3 * r + c] * (b[c] - im.t[c]); }
				d2 += (pb - pa) * (pb - pa);
			}
			depth_num = (1 / depth_min - 1 / depth_max) / (1 / depth_min - 1 / (depth_min + std::sqrt(d2)));
		}
		double* d = &out->depth[4 * i];
		d[0] = depth_min;
		d[1] = (depth_max - depth_min) / (depth_num - 1) / opt.interval_scale;
		d[2] = depth_num;
		d[3] = depth_max;
	}
	return true;
}

namespace {

bool write_text(const path& file, const std::string& text, std::string* error) {
	if (!WriteFileAtomic(file, text.data(), text.size())) return fail(error, "cannot write " + file.string());
	return true;
}

std::string cam_text(const ConvertedCameras& c, size_t i) {
	std::string s = "extrinsic\n";
	for (int r = 0; r < 4; ++r) {
		for (int k = 0; k < 4; ++k) s += PyFloatStr(c.extrinsic[16 * i + 4 * r + k]) + " ";
		s += "\n";
	}
	s += "\nintrinsic\n";
	for (int r = 0; r < 3; ++r) {
		for (int k = 0; k < 3; ++k) s += PyFloatStr(c.intrinsic[9 * i + 3 * r + k]) + " ";
		s += "\n";
	}
	char line[256];
	snprintf(line, sizeof(line), "\n%f %f %f %f\n", c.depth[4 * i], c.depth[4 * i + 1], c.depth[4 * i + 2], c.depth[4 * i + 3]);
	return s + line;
}

bool has_ext(const path& file, std::initializer_list<const char*> exts) {
	std::string e = file.extension().string();
	for (char& c : e) c = (char)tolower((unsigned char)c);
	for (const char* x : exts)
		if (e == x) return true;
	return false;
}

// cv::imread(IMREAD_COLOR) of an input: B, G, R, a grey file replicated
bool read_input(const path& file, const ConvertOptions& opt, Mat* bgr, std::string* error) {
	if (has_ext(file, { ".jpg", ".jpeg" })) {
		if (!opt.on_gpu) {
			*bgr = DecodeJpeg(file, 3);
			if (bgr->empty()) return fail(error, file.string() + ": not a readable baseline JPEG");
			return true;
		}
		std::vector<uint8_t> bytes;
		{
			std::ifstream in(file, std::ios::binary);
			bytes.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
		}
		if (bytes.empty()) return fail(error, file.string() + ": the file is empty or unreadable");
		int w = 0, h = 0;
		if (dvp_jpeg_decode(opt.device, bytes.data(), (long long)bytes.size(), 3, nullptr, 0, &w, &h) != 0) return fail(error, file.string() + ": " + dvp_jpeg_decode_last_error());
		*bgr = Mat(h, w, CV_8UC3);
		if (dvp_jpeg_decode(opt.device, bytes.data(), (long long)bytes.size(), 3, bgr->data, (long long)bgr->step, nullptr, nullptr) != 0) return fail(error, file.string() + ": " + dvp_jpeg_decode_last_error());
		return true;
	}
	if (has_ext(file, { ".ppm", ".pgm" })) {
		*bgr = ReadPnm(file, 3);
		if (bgr->empty()) return fail(error, file.string() + ": not a readable binary PGM / PPM with 255 levels");
		return true;
	}
	return fail(error, file.string() + ": unsupported image format (baseline JPEG, binary PGM and PPM are read)");
}

}   // namespace

bool ConvertColmap(const ConvertOptions& opt, std::string* error) {
	if (!(opt.scale_factor > 0)) return fail(error, "--scale-factor must be positive");
	if (opt.max_d < 0 || opt.max_d == 1) return fail(error, "--max-d must be 0 or at least 2");
	if (!(opt.interval_scale > 0)) return fail(error, "--interval-scale must be positive");
	ColmapModel model;
	if (!ReadColmapModel(opt.colmap_folder / opt.model_dir, opt.model_ext, &model, error)) return false;
	const int n = (int)model.images.size();
	ConvertedCameras cams;
	if (!ConvertCameras(model, opt, &cams, error)) return false;

	// --undistort on: every picture's camera, by image; FOV has no undistortion here
	std::vector<const ColmapCamera*> camera_of((size_t)n, nullptr);
	if (opt.undistort)
		for (int i = 0; i < n; ++i) {
			for (const ColmapCamera& c : model.cameras)
				if (c.id == model.images[(size_t)i].camera_id) camera_of[(size_t)i] = &c;   // (ConvertCameras has met every id)
			if (camera_of[(size_t)i]->model == "FOV") return fail(error, "camera " + std::to_string(camera_of[(size_t)i]->id) + ": --undistort on cannot undistort the FOV camera model (image " + model.images[(size_t)i].name + ")");
		}

	// the sizes first, from the headers: nothing is written when an input is unusable
	const path image_dir = opt.colmap_folder / "images";
	int max_w = 0, max_h = 0;
	if (opt.images)
		for (const ColmapImage& im : model.images) {
			const path file = image_dir / im.name;
			int w = 0, h = 0;
			if (!has_ext(file, { ".jpg", ".jpeg", ".ppm", ".pgm" })) return fail(error, file.string() + ": unsupported image format (baseline JPEG, binary PGM and PPM are read)");
			if (!std::filesystem::exists(file) || !ImageFileSize(file, &w, &h)) return fail(error, file.string() + ": missing, or its header is unreadable");
			max_w = std::max(max_w, w);
			max_h = std::max(max_h, h);
			if (opt.undistort) {
				const ColmapCamera& c = *camera_of[(size_t)(&im - model.images.data())];
				if (c.width != w || c.height != h)
					return fail(error, file.string() + ": the picture is " + std::to_string(w) + " x " + std::to_string(h) + ", its camera " + std::to_string(c.id) + " " + std::to_string(c.width) + " x " +
					                       std::to_string(c.height) + " (--undistort on needs the pictures the model was made from)");
			}
		}

	// view selection
	std::vector<long long> offsets(1, 0), ids, point_ids;
	std::vector<double> xyz;
	for (const ColmapImage& im : model.images) {
		ids.insert(ids.end(), im.point_ids.begin(), im.point_ids.end());
		offsets.push_back((long long)ids.size());
	}
	for (const ColmapPoint& p : model.points) {
		point_ids.push_back(p.id);
		xyz.insert(xyz.end(), p.xyz, p.xyz + 3);
	}
	std::vector<uint32_t> score((size_t)n * n, 0);
	if (opt.on_gpu) {
		if (dvp_view_scores(opt.device, n, offsets.data(), ids.data(), cams.centres.data(), (long long)point_ids.size(), point_ids.data(), xyz.data(), score.data()) != 0)
			return fail(error, dvp_pairs_last_error());
	} else {
		const std::string what = dvppairs::view_scores_serial(n, offsets.data(), ids.data(), cams.centres.data(), (long long)point_ids.size(), point_ids.data(), xyz.data(), score.data());
		if (!what.empty()) return fail(error, "view scores: " + what);
	}

	std::error_code ec;
	std::filesystem::create_directories(opt.save_folder / "cams", ec);
	if (opt.images) std::filesystem::create_directories(opt.save_folder / "images", ec);
	if (opt.sfm) std::filesystem::create_directories(opt.save_folder / "sfm", ec);
	for (int i = 0; i < n; ++i)
		if (!write_text(opt.save_folder / "cams" / (ToFormatIndex(i) + "_cam.txt"), cam_text(cams, (size_t)i), error)) return false;
	if (!write_text(opt.save_folder / "pair.txt", PairText(score.data(), n), error)) return false;

	if (opt.sfm) {
		std::map<long long, size_t> point_at;
		for (size_t k = 0; k < model.points.size(); ++k) point_at[model.points[k].id] = k;
		for (int i = 0; i < n; ++i) {
			const ColmapImage& im = model.images[(size_t)i];
			std::string text;
			for (size_t o = 0; o < im.point_ids.size(); ++o) {
				if (im.point_ids[o] == -1) continue;
				const ColmapPoint& p = model.points[point_at.at(im.point_ids[o])];   // (ConvertCameras has met every id)
				double px = im.xy[2 * o], py = im.xy[2 * o + 1];
				if (opt.undistort) {
					// where the point lies in the undistorted picture: its pinhole projection, fx Xc / Zc + cx with (Xc, Yc, Zc) = R X + t
					const double* e = &cams.extrinsic[16 * (size_t)i];
					const ColmapCamera& cam = *camera_of[(size_t)i];
					const dvpund::Camera pin = dvpund::make_camera(kind_by_name(cam.model)->id, cam.params.data());
					const double xc = e[0] * p.xyz[0] + e[1] * p.xyz[1] + e[2] * p.xyz[2] + e[3], yc = e[4] * p.xyz[0] + e[5] * p.xyz[1] + e[6] * p.xyz[2] + e[7],
					             zc = e[8] * p.xyz[0] + e[9] * p.xyz[1] + e[10] * p.xyz[2] + e[11];
					if (!(zc > 0)) continue;
					px = pin.fx * xc / zc + pin.cx;
					py = pin.fy * yc / zc + pin.cy;
				}
				text += PyFloatStr(px / opt.scale_factor) + " " + PyFloatStr(py / opt.scale_factor) + " " + PyFloatStr(p.xyz[0]) + " " + PyFloatStr(p.xyz[1]) + " " +
				        PyFloatStr(p.xyz[2]) + " " + std::to_string(p.rgb[0]) + " " + std::to_string(p.rgb[1]) + " " + std::to_string(p.rgb[2]) + "\n";
			}
			if (!write_text(opt.save_folder / "sfm" / (ToFormatIndex(i) + ".txt"), text, error)) return false;
		}
	}

	if (!opt.images) return true;
	const int out_w = (int)(max_w / opt.scale_factor), out_h = (int)(max_h / opt.scale_factor);
	if (out_w < 1 || out_h < 1 || out_w > 65535 || out_h > 65535) return fail(error, "the written images would be " + std::to_string(out_w) + " x " + std::to_string(out_h) + " (sizes of 1 ... 65535)");
	std::vector<uint8_t> picture((size_t)out_w * out_h * 3), jpeg;
	for (int i = 0; i < n; ++i) {
		const path file = image_dir / model.images[(size_t)i].name;
		Mat bgr;
		if (!read_input(file, opt, &bgr, error)) return false;
		if (opt.undistort) {
			const ColmapCamera& c = *camera_of[(size_t)i];
			const int kind = kind_by_name(c.model)->id;
			Mat flat(bgr.rows, bgr.cols, CV_8UC3);
			if (opt.on_gpu) {
				if (dvp_undistort_image(opt.device, bgr.data, bgr.cols, bgr.rows, (long long)bgr.step, kind, c.params.data(), kind_by_name(c.model)->num_params, flat.data) != 0)
					return fail(error, file.string() + ": " + dvp_undistort_last_error());
			} else {
				const std::string what = dvpund::check_undistort(bgr.data, bgr.cols, bgr.rows, (long long)bgr.step, kind, c.params.data(), kind_by_name(c.model)->num_params, flat.data);
				if (!what.empty()) return fail(error, file.string() + ": " + what);
				dvpund::undistort_image_serial(dvpund::make_camera(kind, c.params.data()), bgr.data, bgr.cols, bgr.rows, (size_t)bgr.step, flat.data);
			}
			bgr = flat;
		}
		if (opt.on_gpu) {
			if (dvp_convert_image(opt.device, bgr.data, bgr.cols, bgr.rows, (long long)bgr.step, max_w, max_h, out_w, out_h, picture.data()) != 0) return fail(error, file.string() + ": " + dvp_pairs_last_error());
		} else {
			const std::string what = dvppairs::check_convert(bgr.data, bgr.cols, bgr.rows, (long long)bgr.step, max_w, max_h, out_w, out_h, picture.data());
			if (!what.empty()) return fail(error, file.string() + ": " + what);
			dvppairs::convert_image_serial(bgr.data, bgr.cols, bgr.rows, (size_t)bgr.step, max_w, max_h, out_w, out_h, picture.data());
		}
		// cv::imwrite's defaults: three channels, quality 95, 4:2:0
		const long long cap = dvp_jpeg_bound(out_w, out_h, 3);
		jpeg.resize(cap > 0 ? (size_t)cap : 0);
		long long bytes = 0;
		if (dvp_jpeg_encode(opt.device, picture.data(), out_w, out_h, 3, 3ll * out_w, 95, 0, jpeg.data(), cap, &bytes) != 0) return fail(error, file.string() + ": " + dvp_jpeg_last_error());
		const path dst = opt.save_folder / "images" / (ToFormatIndex(i) + ".jpg");
		if (!WriteFileAtomic(dst, jpeg.data(), (size_t)bytes)) return fail(error, "cannot write " + dst.string());
	}
	return true;
}
