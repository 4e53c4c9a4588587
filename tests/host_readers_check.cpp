// host_readers_check — the host's readers of bytes it did not make (csrc/zr_world_doc.cpp: the world document; csrc/zr_asset_files.cpp:
// OBJ and PNG files; both plain C++17, nothing of HIP) run over a corpus that tests/test_host_readers_cpu.py writes, under the sanitizers
// where the machine links them.  The test compiles and runs this; nothing of it is loaded into another process.
//
//   host_readers_check DIR N_PNG N_OBJ
// DIR/docs.bin, little-endian 32-bit words: the number of documents, then per document its length and its bytes.  DIR/png/K.png and
// DIR/obj/K.obj: the files.  Every document handed to the parser is a heap block of exactly its length, so that a read of one byte past
// it is the sanitizer's to report.  One line per case, with a 64-bit FNV-1a hash of what the reader made of it (the test compares it
// with the built library's answer to the same bytes):
//   doc K ok=0 hash=H                       refused; H of the message
//   doc K ok=1 finite=F fixed=X hash=H      accepted; H of the written text.  finite: every float of the parsed world is.  fixed: the
//                                           written text parses, is written as the same text again, and the world's diff against itself
//                                           is 0 - required of every finite document (a number beyond the range of a float parses to an
//                                           infinity, which is written as "inf" and refused on the way back: counted, not required)
//   png K ok=1 w=W h=H hash=H               four channels, W * H * 4 bytes, 1 ... 16 384 on a side; H of the pixels
//   obj K ok=1 nv=V ni=I hash=H             I a multiple of three, every index below V; H of vertices, then indices
//   png K ok=0 / obj K ok=0                 refused (with a message)
// Exit status 1 when a case broke what is required of it.
#include "zr_asset_files.h"
#include "zr_world_doc.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

static uint64_t fnv1a(uint64_t h, const void* data, size_t n)
{
    const uint8_t* p = (const uint8_t*)data;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001B3ull; }
    return h;
}
static const uint64_t kFnvBasis = 0xCBF29CE484222325ull;

static bool parse_exact(const char* src, size_t n, ZrWorld& w, std::string& err)      // from a heap block of exactly n bytes (n == 0: one nobody may read)
{
    std::unique_ptr<char[]> block(new char[n ? n : 1]);
    if (n) memcpy(block.get(), src, n);
    return zr_world_parse(block.get(), n, w, err);
}

static bool finite_lights(const std::vector<ZrLightDesc>& ls)
{
    for (const ZrLightDesc& l : ls) {
        const float v[15] = { l.Position[0], l.Position[1], l.Position[2], l.Color[0], l.Color[1], l.Color[2], l.Intensity, l.Direction[0],
                              l.Direction[1], l.Direction[2], l.Radius, l.ExtraData[0], l.ExtraData[1], l.ExtraData[2], l.ExtraData[3] };
        for (float f : v) if (!std::isfinite(f)) return false;
    }
    return true;
}

static bool finite_world(const ZrWorld& w)
{
    const zr_camera& c = w.MainCamera;
    const float cam[10] = { c.Position[0], c.Position[1], c.Position[2], c.Lookat[0], c.Lookat[1], c.Lookat[2], c.Speed, c.FOV, c.zNear, c.zFar };
    for (float f : cam) if (!std::isfinite(f)) return false;
    for (const ZrObjectDesc& d : w.ObjectDescs) {
        const float v[10] = { d.MinRadius, d.MaxRadius, d.MinRotYaw, d.MaxRotYaw, d.MinRotRoll, d.MaxRotRoll, d.MinRotPitch, d.MaxRotPitch, d.MinPScale, d.MaxPScale };
        for (float f : v) if (!std::isfinite(f)) return false;
    }
    return finite_lights(w.DirectionalLights) && finite_lights(w.PointLights) && finite_lights(w.SpotLights);
}

struct DocTally { unsigned n = 0, accepted = 0, refused = 0, nonfinite = 0, broken = 0; };

static void check_doc(unsigned k, const char* src, size_t n, DocTally& T)
{
    ZrWorld w1, w2; std::string err;
    ++T.n;
    if (!parse_exact(src, n, w1, err)) {
        ++T.refused;
        if (err.empty() || w1.loaded) ++T.broken;
        printf("doc %u ok=0 hash=%016llx\n", k, (unsigned long long)fnv1a(kFnvBasis, err.data(), err.size()));
        return;
    }
    ++T.accepted;
    const std::string t1 = zr_world_to_json(w1);
    const bool finite = finite_world(w1), again = parse_exact(t1.data(), t1.size(), w2, err);
    const bool fixed = again && zr_world_to_json(w2) == t1 && zr_world_diff(w1, w1) == 0u && zr_world_diff(w2, w2) == 0u;
    if (!finite) ++T.nonfinite;
    else if (!fixed) ++T.broken;
    if (!w1.loaded) ++T.broken;
    printf("doc %u ok=1 finite=%d fixed=%d hash=%016llx\n", k, (int)finite, (int)fixed, (unsigned long long)fnv1a(kFnvBasis, t1.data(), t1.size()));
}

static bool read_docs(const std::string& path, DocTally& T)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint32_t count = 0, len = 0;
    bool ok = fread(&count, 4, 1, f) == 1 && count <= (1u << 20);
    std::vector<char> doc;
    for (uint32_t k = 0; ok && k < count; ++k) {
        ok = fread(&len, 4, 1, f) == 1 && len <= (64u << 20);
        if (!ok) break;
        doc.resize(len);
        ok = !len || fread(doc.data(), 1, len, f) == len;
        if (ok) check_doc(k, doc.data(), len, T);
    }
    fclose(f);
    return ok;
}

struct FileTally { unsigned n = 0, accepted = 0, refused = 0, broken = 0; };

static void check_png(unsigned k, const std::string& path, FileTally& T)
{
    std::vector<uint8_t> px; uint32_t w = 0, h = 0; std::string err;
    ++T.n;
    if (!zr_png_load(path, &px, &w, &h, &err)) {
        ++T.refused;
        if (err.empty()) ++T.broken;
        printf("png %u ok=0\n", k);
        return;
    }
    ++T.accepted;
    if (!w || !h || w > 16384u || h > 16384u || px.size() != (size_t)w * h * 4u) ++T.broken;
    printf("png %u ok=1 w=%u h=%u hash=%016llx\n", k, w, h, (unsigned long long)fnv1a(kFnvBasis, px.data(), px.size()));
}

static void check_obj(unsigned k, const std::string& path, FileTally& T)
{
    std::vector<XkVertex> v; std::vector<uint32_t> idx; std::string err;
    ++T.n;
    if (!zr_obj_ingest(path, &v, &idx, &err)) {
        ++T.refused;
        if (err.empty()) ++T.broken;
        printf("obj %u ok=0\n", k);
        return;
    }
    ++T.accepted;
    bool good = idx.size() % 3u == 0u;
    for (uint32_t i : idx) if (i >= v.size()) good = false;
    if (!good) ++T.broken;
    const uint64_t h = fnv1a(fnv1a(kFnvBasis, v.data(), v.size() * sizeof(XkVertex)), idx.data(), idx.size() * 4u);
    printf("obj %u ok=1 nv=%zu ni=%zu hash=%016llx\n", k, v.size(), idx.size(), (unsigned long long)h);
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "host_readers_check DIR N_PNG N_OBJ\n"); return 2; }
    const std::string dir = argv[1];
    const unsigned n_png = (unsigned)strtoul(argv[2], nullptr, 10), n_obj = (unsigned)strtoul(argv[3], nullptr, 10);
    DocTally D; FileTally P, O;
    if (!read_docs(dir + "/docs.bin", D)) { fprintf(stderr, "host_readers_check: cannot read %s/docs.bin\n", dir.c_str()); return 2; }
    for (unsigned k = 0; k < n_png; ++k) check_png(k, dir + "/png/" + std::to_string(k) + ".png", P);
    for (unsigned k = 0; k < n_obj; ++k) check_obj(k, dir + "/obj/" + std::to_string(k) + ".obj", O);
    printf("docs %u accepted %u refused %u nonfinite %u broken %u\n", D.n, D.accepted, D.refused, D.nonfinite, D.broken);
    printf("png %u accepted %u refused %u broken %u\n", P.n, P.accepted, P.refused, P.broken);
    printf("obj %u accepted %u refused %u broken %u\n", O.n, O.accepted, O.refused, O.broken);
    return (D.broken || P.broken || O.broken) ? 1 : 0;
}
