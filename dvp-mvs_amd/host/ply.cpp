// ply.cpp — the vertex reader of `apd --evaluate` (evaluate.h): the PLY files people have (laser scans with doubles, normals and
// colours, meshes with a face element after the vertices) and what ExportPointCloud writes (io.cpp).
#include "evaluate.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

namespace {

struct PlyProperty {
	std::string type, name;
	int size = 0;   // bytes in a binary body; 0: a list
};
struct PlyElement {
	std::string name;
	long long count = 0;
	std::vector<PlyProperty> properties;
};

int ScalarSize(const std::string& t) {
	if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
	if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
	if (t == "int" || t == "uint" || t == "int32" || t == "uint32" || t == "float" || t == "float32") return 4;
	if (t == "double" || t == "float64") return 8;
	return 0;
}
bool IsFloat(const std::string& t) { return t == "float" || t == "float32"; }
bool IsDouble(const std::string& t) { return t == "double" || t == "float64"; }

bool Line(std::istream& in, std::string* line) {
	if (!std::getline(in, *line)) return false;
	if (!line->empty() && line->back() == '\r') line->pop_back();
	return true;
}

}  // namespace

bool ReadPlyVertices(const std::string& file, std::vector<float>* xyz, std::string* error) {
	auto fail = [&](const std::string& what) { xyz->clear(); *error = file + ": " + what; return false; };
	xyz->clear();
	std::ifstream in(file, std::ios::binary);
	if (!in.good()) return fail("cannot be opened");
	std::string line;
	if (!Line(in, &line) || line != "ply") return fail("not a PLY file (the first line is not `ply`)");
	std::string format;
	std::vector<PlyElement> elements;
	bool ended = false;
	while (Line(in, &line)) {
		std::istringstream words(line);
		std::string word;
		if (!(words >> word) || word == "comment" || word == "obj_info") continue;
		if (word == "end_header") { ended = true; break; }
		if (word == "format") { words >> format; continue; }
		if (word == "element") {
			PlyElement e;
			if (!(words >> e.name >> e.count) || e.count < 0) return fail("bad header line `" + line + "`");
			elements.push_back(e);
			continue;
		}
		if (word == "property") {
			if (elements.empty()) return fail("a property before any element");
			PlyProperty p;
			words >> p.type;
			if (p.type == "list") {
				std::string count_type, item_type;
				words >> count_type >> item_type >> p.name;
			} else {
				words >> p.name;
				p.size = ScalarSize(p.type);
				if (p.size == 0) return fail("unknown property type `" + p.type + "`");
			}
			if (p.name.empty()) return fail("bad header line `" + line + "`");
			elements.back().properties.push_back(p);
			continue;
		}
		return fail("bad header line `" + line + "`");
	}
	if (!ended) return fail("the header has no end_header");
	if (format == "binary_big_endian") return fail("format binary_big_endian is not supported (binary_little_endian and ascii are)");
	if (format != "binary_little_endian" && format != "ascii") return fail("unknown format `" + format + "`");
	const bool ascii = format == "ascii";
	size_t v = 0;
	while (v < elements.size() && elements[v].name != "vertex") ++v;
	if (v == elements.size()) return fail("no element vertex");
	for (size_t e = 0; e <= v; ++e)
		for (const PlyProperty& p : elements[e].properties)
			if (p.size == 0) return fail("list property `" + p.name + "` in element " + elements[e].name + (e < v ? ", which comes before element vertex" : "") + " is not supported");
	const PlyElement& vertex = elements[v];
	if (vertex.count > 2147483647ll) return fail("more than 2^31 - 1 vertices");
	int at[3] = { -1, -1, -1 }, offset[3] = { 0, 0, 0 };
	bool wide[3] = { false, false, false };
	int stride = 0;
	for (size_t k = 0; k < vertex.properties.size(); ++k) {
		const PlyProperty& p = vertex.properties[k];
		for (int a = 0; a < 3; ++a)
			if (p.name == std::string(1, "xyz"[a]) && at[a] < 0) {
				if (!IsFloat(p.type) && !IsDouble(p.type)) return fail("property " + p.name + " of element vertex is " + p.type + ", float or double is required");
				at[a] = (int)k;
				offset[a] = stride;
				wide[a] = IsDouble(p.type);
			}
		stride += p.size;
	}
	for (int a = 0; a < 3; ++a)
		if (at[a] < 0) return fail(std::string("element vertex has no property ") + "xyz"[a]);
	// The header's count is not trusted with memory: the vector grows with the vertices that are really there (a truncated file that
	// claims 2^31 - 1 of them is told that its body is short, not handed 25 GB).
	const size_t n = (size_t)vertex.count;
	if (ascii) {
		std::string token;
		for (size_t e = 0; e < v; ++e)
			for (long long i = 0; i < elements[e].count * (long long)elements[e].properties.size(); ++i)
				if (!(in >> token)) return fail("the body is short: it ends inside element " + elements[e].name);
		for (size_t i = 0; i < n; ++i) {
			xyz->resize(3 * (i + 1));
			for (size_t k = 0; k < vertex.properties.size(); ++k) {
				if (!(in >> token)) return fail("the body is short: " + std::to_string(i) + " of " + std::to_string(n) + " vertices");
				for (int a = 0; a < 3; ++a)
					if (at[a] == (int)k) {
						char* end = nullptr;
						const double d = std::strtod(token.c_str(), &end);
						if (end == token.c_str() || *end) return fail("vertex " + std::to_string(i) + ": `" + token + "` is not a number");
						(*xyz)[3 * i + a] = wide[a] ? (float)d : std::strtof(token.c_str(), nullptr);
					}
			}
		}
		return true;
	}
	for (size_t e = 0; e < v; ++e) {
		long long bytes = 0;
		for (const PlyProperty& p : elements[e].properties) bytes += p.size;
		in.ignore((std::streamsize)(bytes * elements[e].count));
		if (!in.good()) return fail("the body is short: it ends inside element " + elements[e].name);
	}
	const size_t chunk = 1 << 16;
	std::vector<char> rows(chunk * (size_t)stride);
	for (size_t first = 0; first < n; first += chunk) {
		const size_t m = n - first < chunk ? n - first : chunk;
		in.read(rows.data(), (std::streamsize)(m * (size_t)stride));
		const size_t got = (size_t)in.gcount() / (size_t)stride;
		if (got < m) return fail("the body is short: " + std::to_string(first + got) + " of " + std::to_string(n) + " vertices");
		xyz->resize(3 * (first + m));
		for (size_t i = 0; i < m; ++i)
			for (int a = 0; a < 3; ++a) {
				const char* src = rows.data() + i * (size_t)stride + offset[a];
				float value;
				if (wide[a]) { double d; memcpy(&d, src, 8); value = (float)d; }
				else memcpy(&value, src, 4);
				(*xyz)[3 * (first + i) + a] = value;
			}
	}
	return true;
}
