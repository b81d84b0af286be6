// prepfiles.cpp — the two files `apd --evaluate` takes for the preparation of the clouds (evaluate.h): --transform, 16 numbers
// separated by whitespace as numpy.savetxt writes a 4 x 4 matrix, and --crop, Open3D's SelectionPolygonVolume JSON, of which
// orthogonal_axis, axis_min, axis_max and bounding_polygon are read and every other key is ignored.  The JSON reader is a small
// recursive descent over the whole grammar (objects, arrays, strings with escapes, numbers, true / false / null); a surrogate pair
// in a \u escape is kept as two code units, which no field read here can hold.  --against-scans takes a MeshLab project (ETH3D's
// scan_alignment.mlp), of which the MLMesh elements' filename attributes and MLMatrix44 bodies are read by a scan over the tags: no
// entities, no CDATA, which neither holds.
#include "evaluate.h"

#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <utility>

static bool ReadWhole(const std::string& file, std::string* text, std::string* error) {
	std::ifstream in(file, std::ios::binary);
	if (!in.good()) { *error = "cannot read " + file; return false; }
	std::stringstream all;
	all << in.rdbuf();
	*text = all.str();
	return true;
}

bool ReadTransformFile(const std::string& file, double m[16], std::string* error) {
	std::string text;
	if (!ReadWhole(file, &text, error)) return false;
	std::stringstream words(text);
	std::string word;
	long long count = 0;
	while (words >> word) {
		char* end = nullptr;
		const double v = std::strtod(word.c_str(), &end);
		if (end == word.c_str() || *end) { *error = file + ": `" + word + "` is not a number"; return false; }
		if (count < 16) m[count] = v;
		++count;
	}
	if (count != 16) { *error = file + " holds " + std::to_string(count) + " numbers; a transform is 16 (4 x 4, row-major)"; return false; }
	dvpcp::Prep p;
	p.has_transform = true;
	for (int k = 0; k < 16; ++k) p.m[k] = m[k];
	const std::string what = dvpcp::check_prep(p);
	if (!what.empty()) { *error = file + ": " + what; return false; }
	return true;
}

// ---- --against-scans: a MeshLab project ----------------------------------------------------------------------------------------------
namespace {

bool XmlSpace(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
bool XmlName(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_' || c == ':' || c == '-' || c == '.'; }

// the attributes of the start tag whose name ends at `at`: name = "value" or 'value'.  Returns the position behind the tag's `>`
// (npos: the tag does not end); *closed = the tag ends with `/>`
size_t XmlAttributes(const std::string& s, size_t at, std::vector<std::pair<std::string, std::string>>* attributes, bool* closed) {
	*closed = false;
	for (;;) {
		while (at < s.size() && XmlSpace(s[at])) ++at;
		if (at >= s.size()) return std::string::npos;
		if (s[at] == '>') return at + 1;
		if (s[at] == '/' || s[at] == '?') { *closed = true; ++at; continue; }
		const size_t first = at;
		while (at < s.size() && XmlName(s[at])) ++at;
		if (at == first) { ++at; continue; }   // (a stray character: skipped)
		const std::string name = s.substr(first, at - first);
		while (at < s.size() && XmlSpace(s[at])) ++at;
		if (at >= s.size() || s[at] != '=') continue;   // (an attribute without a value)
		++at;
		while (at < s.size() && XmlSpace(s[at])) ++at;
		if (at >= s.size() || (s[at] != '"' && s[at] != '\'')) continue;
		const char quote = s[at++];
		const size_t end = s.find(quote, at);
		if (end == std::string::npos) return std::string::npos;
		attributes->emplace_back(name, s.substr(at, end - at));
		at = end + 1;
	}
}

// the next start tag at or behind `at`: its position (npos: none) and name; comments are skipped
size_t XmlNextTag(const std::string& s, size_t at, std::string* name, size_t* name_end) {
	for (;;) {
		at = s.find('<', at);
		if (at == std::string::npos) return at;
		if (s.compare(at, 4, "<!--") == 0) {
			const size_t end = s.find("-->", at + 4);
			if (end == std::string::npos) return end;
			at = end + 3;
			continue;
		}
		size_t k = at + 1;
		while (k < s.size() && XmlName(s[k])) ++k;
		if (k == at + 1) { ++at; continue; }   // an end tag, a declaration, a processing instruction
		*name = s.substr(at + 1, k - at - 1);
		*name_end = k;
		return at;
	}
}

}   // namespace

bool ReadScanProject(const std::string& file, std::vector<ScanEntry>* scans, std::string* error) {
	std::string text;
	if (!ReadWhole(file, &text, error)) return false;
	const size_t slash = file.find_last_of('/');
	const std::string folder = slash == std::string::npos ? "" : file.substr(0, slash + 1);
	scans->clear();
	std::string name;
	size_t name_end = 0, at = 0;
	long long meshes = 0;
	while ((at = XmlNextTag(text, at, &name, &name_end)) != std::string::npos) {
		at = name_end;
		if (name != "MLMesh") continue;
		++meshes;
		std::vector<std::pair<std::string, std::string>> attributes;
		bool closed = false;
		at = XmlAttributes(text, name_end, &attributes, &closed);
		if (at == std::string::npos) { *error = file + ": MLMesh element " + std::to_string(meshes) + " does not end"; return false; }
		ScanEntry entry;
		bool named = false;
		for (const auto& a : attributes)
			if (a.first == "filename" && !named) { entry.name = a.second; named = true; }
		if (!named || entry.name.empty()) { *error = file + ": MLMesh element " + std::to_string(meshes) + " has no filename"; return false; }
		entry.path = entry.name[0] == '/' ? entry.name : folder + entry.name;
		// the element's matrix: the first MLMatrix44 before the element ends or the next MLMesh begins
		size_t matrix = std::string::npos, next = at;
		std::string inner;
		size_t inner_end = 0;
		const size_t limit = closed ? at : text.find("</MLMesh", at);
		while (!closed && (next = XmlNextTag(text, next, &inner, &inner_end)) != std::string::npos && next < limit) {
			if (inner == "MLMesh") break;
			if (inner == "MLMatrix44") { matrix = inner_end; break; }
			next = inner_end;
		}
		if (matrix == std::string::npos) { *error = file + ": the MLMesh " + entry.name + " has no MLMatrix44"; return false; }
		std::vector<std::pair<std::string, std::string>> none;
		bool empty = false;
		const size_t body = XmlAttributes(text, matrix, &none, &empty);
		const size_t body_end = body == std::string::npos ? body : text.find('<', body);
		if (body == std::string::npos || body_end == std::string::npos) { *error = file + ": the MLMatrix44 of " + entry.name + " does not end"; return false; }
		std::stringstream words(empty ? std::string() : text.substr(body, body_end - body));
		std::string word;
		long long count = 0;
		while (words >> word) {
			char* end = nullptr;
			const double v = std::strtod(word.c_str(), &end);
			if (end == word.c_str() || *end) { *error = file + ": the MLMatrix44 of " + entry.name + ": `" + word + "` is not a number"; return false; }
			if (count < 16) entry.m[count] = v;
			++count;
		}
		if (count != 16) { *error = file + ": the MLMatrix44 of " + entry.name + " holds " + std::to_string(count) + " numbers; a transform is 16 (4 x 4, row-major)"; return false; }
		dvpcp::Prep p;
		p.has_transform = true;
		for (int k = 0; k < 16; ++k) p.m[k] = entry.m[k];
		const std::string what = dvpcp::check_prep(p);
		if (!what.empty()) { *error = file + ": the MLMatrix44 of " + entry.name + ": " + what; return false; }
		if (scans->size() == 64) { *error = file + " holds more than 64 scans"; return false; }
		scans->push_back(entry);
		at = body_end;
	}
	if (scans->empty()) { *error = file + " holds no MLMesh element"; return false; }
	return true;
}

namespace {

struct Json {
	enum Type { kNull, kBool, kNumber, kString, kArray, kObject } type = kNull;
	double number = 0.0;
	std::string string;
	std::vector<Json> items;
	std::vector<std::pair<std::string, Json>> fields;
	const Json* field(const char* name) const {
		for (const auto& f : fields)
			if (f.first == name) return &f.second;
		return nullptr;
	}
};

struct JsonReader {
	const std::string& s;
	size_t at = 0;
	std::string what;   // the first error
	int depth = 0;
	explicit JsonReader(const std::string& text) : s(text) {}
	bool fail(const std::string& expected) {
		if (what.empty()) what = "malformed JSON at byte " + std::to_string(at) + ": expected " + expected;
		return false;
	}
	void space() { while (at < s.size() && (s[at] == ' ' || s[at] == '\t' || s[at] == '\n' || s[at] == '\r')) ++at; }
	bool literal(const char* word) {
		const size_t n = strlen(word);
		if (s.compare(at, n, word) != 0) return fail("a value");
		at += n;
		return true;
	}
	bool text(std::string* out) {
		if (at >= s.size() || s[at] != '"') return fail("a string");
		++at;
		for (;;) {
			if (at >= s.size()) return fail("the end of the string");
			const unsigned char c = (unsigned char)s[at++];
			if (c == '"') return true;
			if (c < 0x20) { --at; return fail("no control character in a string"); }
			if (c != '\\') { out->push_back((char)c); continue; }
			if (at >= s.size()) return fail("an escape");
			const char e = s[at++];
			if (e == '"' || e == '\\' || e == '/') out->push_back(e);
			else if (e == 'b') out->push_back('\b');
			else if (e == 'f') out->push_back('\f');
			else if (e == 'n') out->push_back('\n');
			else if (e == 'r') out->push_back('\r');
			else if (e == 't') out->push_back('\t');
			else if (e == 'u') {
				unsigned code = 0;
				for (int k = 0; k < 4; ++k) {
					const char h = at < s.size() ? s[at] : '\0';
					const int d = h >= '0' && h <= '9' ? h - '0' : h >= 'a' && h <= 'f' ? h - 'a' + 10 : h >= 'A' && h <= 'F' ? h - 'A' + 10 : -1;
					if (d < 0) return fail("four hexadecimal digits");
					code = code * 16 + (unsigned)d;
					++at;
				}
				if (code < 0x80) out->push_back((char)code);
				else if (code < 0x800) { out->push_back((char)(0xc0 | (code >> 6))); out->push_back((char)(0x80 | (code & 0x3f))); }
				else { out->push_back((char)(0xe0 | (code >> 12))); out->push_back((char)(0x80 | ((code >> 6) & 0x3f))); out->push_back((char)(0x80 | (code & 0x3f))); }
			}
			else { --at; return fail("a known escape"); }
		}
	}
	bool number(double* out) {
		// JSON's grammar: -? (0 | [1-9][0-9]*) (. [0-9]+)? ([eE] [+-]? [0-9]+)?
		const size_t first = at;
		auto digits = [&]() { const size_t b = at; while (at < s.size() && s[at] >= '0' && s[at] <= '9') ++at; return at > b; };
		if (at < s.size() && s[at] == '-') ++at;
		if (at < s.size() && s[at] == '0') ++at;
		else if (!digits()) return fail("a value");
		if (at < s.size() && s[at] == '.') { ++at; if (!digits()) return fail("digits after the point"); }
		if (at < s.size() && (s[at] == 'e' || s[at] == 'E')) {
			++at;
			if (at < s.size() && (s[at] == '+' || s[at] == '-')) ++at;
			if (!digits()) return fail("digits in the exponent");
		}
		*out = std::strtod(s.substr(first, at - first).c_str(), nullptr);
		return true;
	}
	bool value(Json* v) {
		if (++depth > 64) return fail("at most 64 nested values");
		space();
		if (at >= s.size()) return fail("a value");
		const char c = s[at];
		bool ok = true;
		if (c == '{') {
			v->type = Json::kObject;
			++at;
			space();
			if (at < s.size() && s[at] == '}') ++at;
			else for (;;) {
				space();
				std::string name;
				Json item;
				if (!text(&name)) return false;
				space();
				if (at >= s.size() || s[at] != ':') return fail("`:`");
				++at;
				if (!value(&item)) return false;
				v->fields.emplace_back(std::move(name), std::move(item));
				space();
				if (at < s.size() && s[at] == ',') { ++at; continue; }
				if (at < s.size() && s[at] == '}') { ++at; break; }
				return fail("`,` or `}`");
			}
		} else if (c == '[') {
			v->type = Json::kArray;
			++at;
			space();
			if (at < s.size() && s[at] == ']') ++at;
			else for (;;) {
				Json item;
				if (!value(&item)) return false;
				v->items.push_back(std::move(item));
				space();
				if (at < s.size() && s[at] == ',') { ++at; continue; }
				if (at < s.size() && s[at] == ']') { ++at; break; }
				return fail("`,` or `]`");
			}
		} else if (c == '"') {
			v->type = Json::kString;
			ok = text(&v->string);
		} else if (c == 't') { v->type = Json::kBool; v->number = 1.0; ok = literal("true"); }
		else if (c == 'f') { v->type = Json::kBool; ok = literal("false"); }
		else if (c == 'n') ok = literal("null");
		else { v->type = Json::kNumber; ok = number(&v->number); }
		--depth;
		return ok;
	}
};

}   // namespace

bool ReadCropFile(const std::string& file, dvpcp::Prep* prep, std::string* error) {
	std::string text;
	if (!ReadWhole(file, &text, error)) return false;
	JsonReader reader(text);
	Json root;
	if (reader.value(&root)) {
		reader.space();
		if (reader.at != text.size()) reader.fail("the end of the file");
	}
	if (!reader.what.empty()) { *error = file + ": " + reader.what; return false; }
	if (root.type != Json::kObject) { *error = file + ": malformed JSON at byte 0: expected an object"; return false; }
	const char* names[4] = { "orthogonal_axis", "axis_min", "axis_max", "bounding_polygon" };
	const Json* f[4];
	for (int k = 0; k < 4; ++k) {
		f[k] = root.field(names[k]);
		if (!f[k]) { *error = file + ": the field `" + names[k] + "` is missing"; return false; }
	}
	const std::string& axis = f[0]->string;
	if (f[0]->type != Json::kString || (axis != "X" && axis != "Y" && axis != "Z")) { *error = file + ": orthogonal_axis must be \"X\", \"Y\" or \"Z\""; return false; }
	if (f[1]->type != Json::kNumber || f[2]->type != Json::kNumber) { *error = file + ": axis_min and axis_max must be numbers"; return false; }
	if (f[3]->type != Json::kArray) { *error = file + ": bounding_polygon must be a list of vertices"; return false; }
	const size_t n = f[3]->items.size();
	if (n < (size_t)dvpcp::kMinPolygon) { *error = file + ": bounding_polygon needs at least 3 vertices, got " + std::to_string(n); return false; }
	if (n > (size_t)dvpcp::kMaxPolygon) { *error = file + ": bounding_polygon takes at most 256 vertices, got " + std::to_string(n); return false; }
	prep->polygon.clear();
	for (size_t k = 0; k < n; ++k) {
		const Json& vertex = f[3]->items[k];
		bool ok = vertex.type == Json::kArray && vertex.items.size() == 3;
		for (size_t a = 0; a < 3 && ok; ++a) ok = vertex.items[a].type == Json::kNumber;
		if (!ok) { *error = file + ": bounding_polygon vertex " + std::to_string(k) + " must hold 3 numbers"; return false; }
		for (size_t a = 0; a < 3; ++a) prep->polygon.push_back(vertex.items[a].number);
	}
	prep->crop_axis = axis == "X" ? 0 : axis == "Y" ? 1 : 2;
	prep->axis_min = f[1]->number;
	prep->axis_max = f[2]->number;
	dvpcp::Prep only_crop;
	only_crop.crop_axis = prep->crop_axis;
	only_crop.axis_min = prep->axis_min;
	only_crop.axis_max = prep->axis_max;
	only_crop.polygon = prep->polygon;
	const std::string what = dvpcp::check_prep(only_crop);   // 1e999 reads as inf; axis_min above axis_max
	if (!what.empty()) { *error = file + ": " + what; return false; }
	return true;
}
