// zr_asset_files.cpp — the readers of files the library did not write: OBJ meshes and PNG images, and the check every file name of a
// world payload passes first.
//
//   zr_obj_ingest          LoadMeshAsset (OBJ branch)            ZE:6899-6948  normals indexed by POSITION index, v flipped, dedupe on the record
//   zr_png_load            LoadTextureAsset (stbi_load, 4 ch.)   ZE:6882-6896  own PNG reader (zlib inflate); stb_image is not in the tree
//
// A livelink world names these files: a damaged or hostile one comes back as an error (or as some image / mesh).  Plain C++17, nothing of
// HIP: tests/host_readers_check.cpp runs this file on the CPU, under the sanitizers.
#include "zr_asset_files.h"

#include <zlib.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>

// Names that arrive in a (possibly unauthenticated) world payload - CubemapFileNames, SkydomeFileName, BackgroundFileName, ProfabName -
// must stay inside the content tree: no absolute path, no ".." component, no NUL.
bool zr_payload_name_ok(const std::string& name)
{
    if (name.empty() || name[0] == '/' || name[0] == '\\' || name.find('\0') != std::string::npos) return false;
    if (name.size() > 1 && name[1] == ':') return false;                       // drive letter
    size_t b = 0;
    while (b <= name.size()) {
        size_t e = name.find_first_of("/\\", b);
        if (e == std::string::npos) e = name.size();
        if (name.compare(b, e - b, "..") == 0) return false;
        b = e + 1;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ OBJ

namespace {

struct ObjData { std::vector<float> pos, nrm, uv; std::vector<int> corners; /* (v, vt, vn) triples, 3 corners per triangle */ };

// tinyobjloader's reading of the few statements the engine's meshes use: v, vn, vt, f (v, v/vt, v//vn, v/vt/vn; 1-based, negative =
// relative to the end; polygons as a fan).  Everything else (o, g, s, usemtl, mtllib, comments) is skipped.
bool parse_obj(const std::string& path, ObjData* o, std::string* err)
{
    std::ifstream in(path);
    if (!in) { *err = "[LoadMeshAsset] Fail to load obj: cannot open " + path; return false; }
    std::string line;
    auto fix = [](long i, size_t n) -> int { return i > 0 ? (int)(i - 1) : (i < 0 ? (int)((long)n + i) : -1); };
    while (std::getline(in, line)) {
        const char* s = line.c_str();
        while (*s == ' ' || *s == '\t') ++s;
        if (s[0] == 'v' && (s[1] == ' ' || s[1] == '\t')) {
            char* e = nullptr; const char* q = s + 1;
            for (int k = 0; k < 3; ++k) { o->pos.push_back((float)strtod(q, &e)); q = e; }
        } else if (s[0] == 'v' && s[1] == 'n' && (s[2] == ' ' || s[2] == '\t')) {
            char* e = nullptr; const char* q = s + 2;
            for (int k = 0; k < 3; ++k) { o->nrm.push_back((float)strtod(q, &e)); q = e; }
        } else if (s[0] == 'v' && s[1] == 't' && (s[2] == ' ' || s[2] == '\t')) {
            char* e = nullptr; const char* q = s + 2;
            for (int k = 0; k < 2; ++k) { const double v = strtod(q, &e); o->uv.push_back(e == q ? 0.0f : (float)v); q = e; }
        } else if (s[0] == 'f' && (s[1] == ' ' || s[1] == '\t')) {
            std::vector<int> poly;
            const char* q = s + 1;
            for (;;) {
                while (*q == ' ' || *q == '\t' || *q == '\r') ++q;
                if (!*q) break;
                char* e = nullptr;
                long vi = strtol(q, &e, 10), ti = 0, ni = 0;
                if (e == q) break;
                q = e;
                if (*q == '/') { ++q; if (*q != '/') { ti = strtol(q, &e, 10); q = e; } if (*q == '/') { ++q; ni = strtol(q, &e, 10); q = e; } }
                poly.push_back(fix(vi, o->pos.size() / 3)); poly.push_back(fix(ti, o->uv.size() / 2)); poly.push_back(fix(ni, o->nrm.size() / 3));
            }
            const size_t nc = poly.size() / 3;
            for (size_t k = 1; k + 1 < nc; ++k)
                for (size_t c : { (size_t)0, k, k + 1 }) { o->corners.push_back(poly[3 * c]); o->corners.push_back(poly[3 * c + 1]); o->corners.push_back(poly[3 * c + 2]); }
        }
    }
    return true;
}

struct VKey { uint32_t w[11]; bool operator<(const VKey& b) const { return memcmp(w, b.w, sizeof w) < 0; } };

}  // namespace

// LoadMeshAsset, ZE:6899-6948.  Quirks kept: attrib.normals is indexed by the POSITION index (ZE:6927-6931), uv.v becomes 1 - v
// (ZE:6937), colour (1, 1, 1), vertices deduplicated on the whole record.
bool zr_obj_ingest(const std::string& path, std::vector<XkVertex>* v, std::vector<uint32_t>* idx, std::string* err)
{
    ObjData o;
    if (!parse_obj(path, &o, err)) return false;
    if (o.nrm.empty() || o.uv.empty()) { *err = "[LoadMeshAsset] " + path + ": the engine's loader indexes attrib.normals and attrib.texcoords unconditionally"; return false; }
    const size_t np = o.pos.size() / 3, nn = o.nrm.size() / 3, nt = o.uv.size() / 2;
    std::map<VKey, uint32_t> uniq;
    for (size_t k = 0; k + 2 < o.corners.size(); k += 3) {
        const int vi = o.corners[k], ti = o.corners[k + 1];
        if (vi < 0 || (size_t)vi >= np || ti < 0 || (size_t)ti >= nt) { *err = "[LoadMeshAsset] " + path + ": face index out of range"; return false; }
        const size_t ni = (size_t)vi < nn ? (size_t)vi : nn - 1;
        XkVertex x;
        for (int a = 0; a < 3; ++a) { x.Position[a] = o.pos[3 * (size_t)vi + a]; x.Normal[a] = o.nrm[3 * ni + a]; x.Color[a] = 1.0f; }
        x.TexCoord[0] = o.uv[2 * (size_t)ti]; x.TexCoord[1] = 1.0f - o.uv[2 * (size_t)ti + 1];
        VKey key; memcpy(key.w, &x, sizeof key.w);
        auto it = uniq.find(key);
        if (it == uniq.end()) { it = uniq.emplace(key, (uint32_t)v->size()).first; v->push_back(x); }
        idx->push_back(it->second);
    }
    if (idx->empty()) { *err = "[LoadMeshAsset] " + path + ": no faces"; return false; }
    return true;
}

// ------------------------------------------------------------------------------------------------ PNG

namespace {

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
int paeth(int a, int b, int c) { const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c); return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }

// reverse the scanline filters of one (sub-)image in place: rows of `stride` bytes, each preceded by its filter byte
bool unfilter(uint8_t* data, size_t rows, size_t stride, size_t bpp)
{
    std::vector<uint8_t> zero(stride, 0);
    for (size_t y = 0; y < rows; ++y) {
        uint8_t* row = data + y * (stride + 1);
        const uint8_t ft = row[0];
        uint8_t* cur = row + 1;
        const uint8_t* up = y ? row - stride : zero.data();
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = up[i], c = i >= bpp ? up[i - bpp] : 0;
            switch (ft) {
            case 0: break;
            case 1: cur[i] = (uint8_t)(cur[i] + a); break;
            case 2: cur[i] = (uint8_t)(cur[i] + b); break;
            case 3: cur[i] = (uint8_t)(cur[i] + ((a + b) >> 1)); break;
            case 4: cur[i] = (uint8_t)(cur[i] + paeth(a, b, c)); break;
            default: return false;
            }
        }
    }
    return true;
}

}  // namespace

// stbi_load(path, &w, &h, &n, STBI_rgb_alpha) for PNG files: 8-bit RGBA out.  Grey, grey+alpha, RGB, RGBA and palette images, bit
// depths 1-16 (16-bit samples keep their high byte), tRNS (palette alpha, or a colour key), Adam7 interlacing.
bool zr_png_load(const std::string& path, std::vector<uint8_t>* rgba, uint32_t* W, uint32_t* H, std::string* err)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) { *err = "[LoadTextureAsset] Failed to load texture image:" + path; return false; }
    std::vector<uint8_t> f((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
    if (f.size() < 8 + 25 || memcmp(f.data(), sig, 8)) { *err = "[LoadTextureAsset] not a PNG file:" + path; return false; }
    uint32_t w = 0, h = 0; int depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> idat, plte, trns;
    for (size_t p = 8; p + 12 <= f.size();) {
        const uint32_t n = be32(&f[p]);
        if (p + 12 + (size_t)n > f.size()) break;
        const char* t = (const char*)&f[p + 4];
        const uint8_t* d = &f[p + 8];
        if (!memcmp(t, "IHDR", 4) && n >= 13) { w = be32(d); h = be32(d + 4); depth = d[8]; ctype = d[9]; interlace = d[12]; }
        else if (!memcmp(t, "PLTE", 4)) plte.assign(d, d + n);
        else if (!memcmp(t, "tRNS", 4)) trns.assign(d, d + n);
        else if (!memcmp(t, "IDAT", 4)) idat.insert(idat.end(), d, d + n);
        else if (!memcmp(t, "IEND", 4)) break;
        p += 12 + (size_t)n;
    }
    const int ch = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!w || !h || w > 16384 || h > 16384 || !ch || (depth != 1 && depth != 2 && depth != 4 && depth != 8 && depth != 16) ||
        (ctype == 3 && (depth == 16 || plte.empty())) || ((ctype == 2 || ctype == 4 || ctype == 6) && depth < 8) || interlace > 1) {
        *err = "[LoadTextureAsset] unsupported PNG header:" + path; return false;
    }
    const size_t bits = (size_t)ch * depth, bpp = std::max<size_t>(1, bits / 8);
    // sub-images: the whole picture, or the seven Adam7 passes
    struct Pass { uint32_t x0, y0, dx, dy; };
    std::vector<Pass> passes;
    if (!interlace) passes.push_back({ 0, 0, 1, 1 });
    else passes = { { 0, 0, 8, 8 }, { 4, 0, 8, 8 }, { 0, 4, 4, 8 }, { 2, 0, 4, 4 }, { 0, 2, 2, 4 }, { 1, 0, 2, 2 }, { 0, 1, 1, 2 } };
    size_t raw_size = 0;
    for (const Pass& ps : passes) {
        const size_t pw = (w + ps.dx - 1 - ps.x0) / ps.dx, ph = (h + ps.dy - 1 - ps.y0) / ps.dy;
        if (pw && ph) raw_size += ph * (1 + (pw * bits + 7) / 8);
    }
    std::vector<uint8_t> raw(raw_size);
    uLongf got = (uLongf)raw.size();
    const int zrc = uncompress(raw.data(), &got, idat.data(), (uLong)idat.size());
    if (zrc != Z_OK || got != raw.size()) { *err = "[LoadTextureAsset] corrupt PNG data:" + path; return false; }
    rgba->assign((size_t)w * h * 4, 0);
    auto sample = [&](const uint8_t* row, size_t i) -> uint32_t {     // i-th sample of a row, as a `depth`-bit integer
        if (depth == 8) return row[i];
        if (depth == 16) return (uint32_t)row[2 * i] << 8 | row[2 * i + 1];
        const size_t bit = i * (size_t)depth;
        return (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1u << depth) - 1u);
    };
    auto to8 = [&](uint32_t v) -> uint8_t {      // stb_image: 16 bit -> high byte; 1/2/4 bit grey -> scaled to 0..255
        if (depth == 16) return (uint8_t)(v >> 8);
        if (depth == 8) return (uint8_t)v;
        return (uint8_t)(v * (255u / ((1u << depth) - 1u)));
    };
    size_t off = 0;
    for (const Pass& ps : passes) {
        const size_t pw = (w + ps.dx - 1 - ps.x0) / ps.dx, ph = (h + ps.dy - 1 - ps.y0) / ps.dy;
        if (!pw || !ph) continue;
        const size_t stride = (pw * bits + 7) / 8;
        if (!unfilter(raw.data() + off, ph, stride, bpp)) { *err = "[LoadTextureAsset] bad PNG filter:" + path; return false; }
        for (size_t y = 0; y < ph; ++y) {
            const uint8_t* row = raw.data() + off + y * (stride + 1) + 1;
            for (size_t x = 0; x < pw; ++x) {
                uint8_t* o = rgba->data() + (((size_t)ps.y0 + y * ps.dy) * w + ps.x0 + x * ps.dx) * 4;
                switch (ctype) {
                case 0: { const uint32_t g = sample(row, x); o[0] = o[1] = o[2] = to8(g);
                          o[3] = (trns.size() >= 2 && g == ((uint32_t)trns[0] << 8 | trns[1])) ? 0 : 255; break; }
                case 2: { const uint32_t r = sample(row, 3 * x), g = sample(row, 3 * x + 1), b = sample(row, 3 * x + 2);
                          o[0] = to8(r); o[1] = to8(g); o[2] = to8(b);
                          o[3] = (trns.size() >= 6 && r == ((uint32_t)trns[0] << 8 | trns[1]) && g == ((uint32_t)trns[2] << 8 | trns[3]) &&
                                  b == ((uint32_t)trns[4] << 8 | trns[5])) ? 0 : 255; break; }
                case 3: { const uint32_t i = sample(row, x);
                          if (3 * (size_t)i + 2 < plte.size()) { o[0] = plte[3 * i]; o[1] = plte[3 * i + 1]; o[2] = plte[3 * i + 2]; }
                          o[3] = i < trns.size() ? trns[i] : 255; break; }
                case 4: { o[0] = o[1] = o[2] = to8(sample(row, 2 * x)); o[3] = to8(sample(row, 2 * x + 1)); break; }
                default: { for (int k = 0; k < 4; ++k) o[k] = to8(sample(row, 4 * x + (size_t)k)); break; }
                }
            }
        }
        off += ph * (stride + 1);
    }
    *W = w; *H = h;
    return true;
}
