// zr_world_doc.cpp — the world document: a minimal JSON parser, XkWorld's schema read with rapidjson's strictness, the writer, the
// diff predicates and the instance generator.
//
// Replaces XkWorld::Load / Save / Reset (ZE:1051-1290, rapidjson) and XkObjectDesc::GenerateInstance (ZE:573-603).  The payload arrives
// over TCP from an unauthenticated client (zr_livelink.cpp) and is parsed on the listener thread: nothing here trusts a byte of it.
// Plain C++17, nothing of HIP: tests/host_readers_check.cpp runs this file on the CPU, under the sanitizers.
#include "zr_world_doc.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>

#define XK_WORLD_MAX_INSTANCES_PER_OBJECT 4194304u     // 2^22 per ObjectDesc (the sample scene uses 10 000); bigger scenes use zr_object_add

// ------------------------------------------------------------------------------------------------ minimal JSON

namespace {

struct JValue;
using JPtr = std::unique_ptr<JValue>;
struct JValue {
    enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
    bool b = false; double num = 0; bool is_int = false;
    std::string str;
    std::vector<JPtr> arr;
    std::vector<std::pair<std::string, JPtr>> obj;
    const JValue* get(const char* key) const { for (auto& kv : obj) if (kv.first == key) return kv.second.get(); return nullptr; }
};

struct JParser {
    const char* p; const char* end; std::string err;
    void ws() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p; }
    bool fail(const char* m) { if (err.empty()) err = m; return false; }
    bool parse_string(std::string& out)
    {
        if (p >= end || *p != '"') return fail("expected string");
        ++p;
        while (p < end && *p != '"') {
            if (*p == '\\') {
                if (++p >= end) return fail("bad escape");
                switch (*p) {
                case '"': out += '"'; break; case '\\': out += '\\'; break; case '/': out += '/'; break;
                case 'b': out += '\b'; break; case 'f': out += '\f'; break; case 'n': out += '\n'; break;
                case 'r': out += '\r'; break; case 't': out += '\t'; break;
                case 'u': {
                    if (end - p < 5) return fail("bad \\u escape");
                    unsigned cp = 0;
                    for (int i = 1; i <= 4; ++i) {
                        char ch = p[i]; cp <<= 4;
                        if (ch >= '0' && ch <= '9') cp |= (unsigned)(ch - '0');
                        else if (ch >= 'a' && ch <= 'f') cp |= (unsigned)(ch - 'a' + 10);
                        else if (ch >= 'A' && ch <= 'F') cp |= (unsigned)(ch - 'A' + 10);
                        else return fail("bad \\u escape");
                    }
                    p += 4;
                    if (cp < 0x80) out += (char)cp;
                    else if (cp < 0x800) { out += (char)(0xC0 | (cp >> 6)); out += (char)(0x80 | (cp & 0x3F)); }
                    else { out += (char)(0xE0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F)); }
                    break;
                }
                default: return fail("bad escape");
                }
                ++p;
            } else out += *p++;
        }
        if (p >= end) return fail("unterminated string");
        ++p;
        return true;
    }
    bool parse(JValue& v, int depth = 0)
    {
        if (depth > 64) return fail("nesting too deep");
        ws();
        if (p >= end) return fail("unexpected end");
        if (*p == '{') {
            v.kind = JValue::Obj; ++p; ws();
            if (p < end && *p == '}') { ++p; return true; }
            for (;;) {
                ws(); std::string k;
                if (!parse_string(k)) return false;
                ws(); if (p >= end || *p != ':') return fail("expected ':'");
                ++p;
                JPtr c(new JValue());
                if (!parse(*c, depth + 1)) return false;
                v.obj.emplace_back(std::move(k), std::move(c));
                ws(); if (p >= end) return fail("unexpected end");
                if (*p == ',') { ++p; continue; }
                if (*p == '}') { ++p; return true; }
                return fail("expected ',' or '}'");
            }
        }
        if (*p == '[') {
            v.kind = JValue::Arr; ++p; ws();
            if (p < end && *p == ']') { ++p; return true; }
            for (;;) {
                JPtr c(new JValue());
                if (!parse(*c, depth + 1)) return false;
                v.arr.push_back(std::move(c));
                ws(); if (p >= end) return fail("unexpected end");
                if (*p == ',') { ++p; continue; }
                if (*p == ']') { ++p; return true; }
                return fail("expected ',' or ']'");
            }
        }
        if (*p == '"') { v.kind = JValue::Str; return parse_string(v.str); }
        if (end - p >= 4 && !strncmp(p, "true", 4)) { v.kind = JValue::Bool; v.b = true; p += 4; return true; }
        if (end - p >= 5 && !strncmp(p, "false", 5)) { v.kind = JValue::Bool; v.b = false; p += 5; return true; }
        if (end - p >= 4 && !strncmp(p, "null", 4)) { v.kind = JValue::Null; p += 4; return true; }
        const char* s = p;
        if (p < end && *p == '-') ++p;
        bool digits = false, isint = true;
        while (p < end && *p >= '0' && *p <= '9') { ++p; digits = true; }
        if (p < end && *p == '.') { isint = false; ++p; while (p < end && *p >= '0' && *p <= '9') { ++p; digits = true; } }
        if (p < end && (*p == 'e' || *p == 'E')) { isint = false; ++p; if (p < end && (*p == '+' || *p == '-')) ++p; while (p < end && *p >= '0' && *p <= '9') ++p; }
        if (!digits) return fail("invalid value");
        v.kind = JValue::Num; v.is_int = isint; v.num = strtod(std::string(s, p).c_str(), nullptr);
        return true;
    }
};

struct Reader {       // typed access with rapidjson-like strictness: a missing key or wrong type is an error, not a default
    std::string err;
    const JValue* need(const JValue* o, const char* k, JValue::Kind kind)
    {
        const JValue* v = (o && o->kind == JValue::Obj) ? o->get(k) : nullptr;
        if (!v) { if (err.empty()) err = std::string("missing key '") + k + "'"; return nullptr; }
        if (v->kind != kind) { if (err.empty()) err = std::string("wrong type for key '") + k + "'"; return nullptr; }
        return v;
    }
    float f(const JValue* o, const char* k) { const JValue* v = need(o, k, JValue::Num); return v ? (float)v->num : 0.0f; }
    uint32_t u(const JValue* o, const char* k)
    {
        const JValue* v = need(o, k, JValue::Num);
        if (v && (!v->is_int || v->num < 0 || v->num > 4294967295.0)) { if (err.empty()) err = std::string("key '") + k + "' is not a uint"; return 0; }
        return v ? (uint32_t)v->num : 0u;
    }
    bool b(const JValue* o, const char* k) { const JValue* v = need(o, k, JValue::Bool); return v ? v->b : false; }
    std::string s(const JValue* o, const char* k) { const JValue* v = need(o, k, JValue::Str); return v ? v->str : std::string(); }
    void fa(const JValue* o, const char* k, float* dst, size_t n)
    {
        const JValue* v = need(o, k, JValue::Arr);
        if (!v) return;
        if (v->arr.size() < n) { if (err.empty()) err = std::string("array '") + k + "' too short"; return; }
        for (size_t i = 0; i < n; ++i) {
            if (v->arr[i]->kind != JValue::Num) { if (err.empty()) err = std::string("array '") + k + "' holds a non-number"; return; }
            dst[i] = (float)v->arr[i]->num;
        }
    }
};

void world_reset(ZrWorld& w)     // XkWorld::Reset, ZE:1265-1290
{
    w = ZrWorld();
    w.EnableSkydome = true; w.OverrideSkydome = true; w.SkydomeFileName = "Content/Textures/skydome.png";
    w.OverrideCubemap = true;
    const char* cm[6] = { "Content/Textures/cubemap_X0.png", "Content/Textures/cubemap_X1.png", "Content/Textures/cubemap_Y2.png",
                          "Content/Textures/cubemap_Y3.png", "Content/Textures/cubemap_Z4.png", "Content/Textures/cubemap_Z5.png" };
    for (int i = 0; i < 6; ++i) w.CubemapFileNames[i] = cm[i];
    w.EnableBackground = true; w.OverrideBackground = true; w.BackgroundFileName = "Content/Textures/background.png";
    const zr_camera cam = { { 5.0f, 5.0f, 5.0f }, { 0.0f, 0.0f, 0.0f }, 2.5f, 45.0f, 0.1f, 45.0f };   // ResetToFocus, ZE:879-887
    w.MainCamera = cam;
}

// PCG-XSH-RR 64/32; stands in for mt19937(std::rand()) of XkObjectDesc::RandRange (ZE:592-603), which is libc-specific
struct Pcg32 {
    uint64_t state, inc;
    explicit Pcg32(uint64_t seed, uint64_t seq = 54) { state = 0; inc = (seq << 1) | 1; next(); state += seed; next(); }
    uint32_t next()
    {
        const uint64_t old = state;
        state = old * 6364136223846793005ull + inc;
        const uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27), rot = (uint32_t)(old >> 59);
        return (xs >> rot) | (xs << ((32 - rot) & 31));
    }
    float unit() { return (float)(next() >> 8) * 5.9604644775390625e-8f; }
    float range(float a, float b) { return a + (b - a) * unit(); }
};

bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }
bool same_lights(const std::vector<ZrLightDesc>& a, const std::vector<ZrLightDesc>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(ZrLightDesc)) == 0);
}
bool same_desc(const ZrObjectDesc& a, const ZrObjectDesc& b)
{
    return a.RenderFlags == b.RenderFlags && a.ProfabName == b.ProfabName && a.InstanceCount == b.InstanceCount &&
           same_bits(a.MinRadius, b.MinRadius) && same_bits(a.MaxRadius, b.MaxRadius) && same_bits(a.MinRotYaw, b.MinRotYaw) &&
           same_bits(a.MaxRotYaw, b.MaxRotYaw) && same_bits(a.MinRotRoll, b.MinRotRoll) && same_bits(a.MaxRotRoll, b.MaxRotRoll) &&
           same_bits(a.MinRotPitch, b.MinRotPitch) && same_bits(a.MaxRotPitch, b.MaxRotPitch) && same_bits(a.MinPScale, b.MinPScale) &&
           same_bits(a.MaxPScale, b.MaxPScale);
}

void jnum(std::string& o, float v)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.9g", (double)v);
    std::string s(buf);
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";   // rapidjson writes doubles with a fraction
    o += s;
}
void jstr(std::string& o, const std::string& s)
{
    o += '"';
    for (char ch : s) {
        switch (ch) {
        case '"': o += "\\\""; break; case '\\': o += "\\\\"; break; case '\n': o += "\\n"; break; case '\r': o += "\\r"; break;
        case '\t': o += "\\t"; break;
        default: if ((unsigned char)ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04X", ch); o += b; } else o += ch;
        }
    }
    o += '"';
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the document read, written, compared

// XkWorld::Load, ZE:1051-1147.  Returns false with `err` set on a parse or schema error.
bool zr_world_parse(const char* utf8, size_t len, ZrWorld& w, std::string& err)
{
    world_reset(w);
    JParser jp{ utf8, utf8 + len, {} };
    JValue root;
    if (!jp.parse(root)) { err = "[WORLD] JSON parse error: " + jp.err; return false; }
    jp.ws();
    if (jp.p != jp.end) { err = "[WORLD] JSON parse error: trailing characters"; return false; }
    if (root.kind != JValue::Obj) { err = "[WORLD] JSON parse error: document is not an object"; return false; }
    Reader R;
    const JValue* cam = R.need(&root, "MainCamera", JValue::Obj);
    R.fa(cam, "Position", w.MainCamera.Position, 3); R.fa(cam, "Lookat", w.MainCamera.Lookat, 3);
    w.MainCamera.FOV = R.f(cam, "FOV"); w.MainCamera.Speed = R.f(cam, "Speed");
    w.MainCamera.zNear = R.f(cam, "zNear"); w.MainCamera.zFar = R.f(cam, "zFar");
    const JValue* sky = R.need(&root, "Skydome", JValue::Obj);
    w.EnableSkydome = R.b(sky, "EnableSkydome"); w.OverrideSkydome = R.b(sky, "OverrideSkydome");
    w.SkydomeFileName = R.s(sky, "SkydomeFileName"); w.OverrideCubemap = R.b(sky, "OverrideCubemap");
    if (const JValue* names = R.need(sky, "CubemapFileNames", JValue::Arr)) {
        if (names->arr.size() > 6) { if (R.err.empty()) R.err = "CubemapFileNames has more than 6 entries"; }
        else for (size_t i = 0; i < names->arr.size(); ++i) {
            if (names->arr[i]->kind != JValue::Str) { if (R.err.empty()) R.err = "CubemapFileNames holds a non-string"; break; }
            w.CubemapFileNames[i] = names->arr[i]->str;
        }
    }
    const JValue* bg = R.need(&root, "Background", JValue::Obj);
    w.EnableBackground = R.b(bg, "EnableBackground"); w.OverrideBackground = R.b(bg, "OverrideBackground");
    w.BackgroundFileName = R.s(bg, "BackgroundFileName");
    auto lights = [&](const char* key, std::vector<ZrLightDesc>& out) {
        const JValue* a = R.need(&root, key, JValue::Arr);
        if (!a) return;
        for (auto& e : a->arr) {
            ZrLightDesc l; memset(&l, 0, sizeof l);
            const JValue* o = e.get();
            if (o->kind != JValue::Obj) { if (R.err.empty()) R.err = std::string(key) + " holds a non-object"; return; }
            R.fa(o, "Position", l.Position, 3); l.Type = R.u(o, "Type"); R.fa(o, "Color", l.Color, 3);
            l.Intensity = R.f(o, "Intensity"); R.fa(o, "Direction", l.Direction, 3); l.Radius = R.f(o, "Radius");
            R.fa(o, "ExtraData", l.ExtraData, 4);
            out.push_back(l);
        }
    };
    lights("DirectionalLights", w.DirectionalLights); lights("PointLights", w.PointLights); lights("SpotLights", w.SpotLights);
    if (const JValue* objs = R.need(&root, "Objects", JValue::Arr))
        for (auto& e : objs->arr) {
            const JValue* o = e.get();
            if (o->kind != JValue::Obj) { if (R.err.empty()) R.err = "Objects holds a non-object"; break; }
            ZrObjectDesc d;
            d.RenderFlags = R.u(o, "RenderFlags"); d.ProfabName = R.s(o, "ProfabName"); d.InstanceCount = R.u(o, "InstanceCount");
            d.MinRadius = R.f(o, "MinRadius"); d.MaxRadius = R.f(o, "MaxRadius"); d.MinRotYaw = R.f(o, "MinRotYaw");
            d.MaxRotYaw = R.f(o, "MaxRotYaw"); d.MinRotRoll = R.f(o, "MinRotRoll"); d.MaxRotRoll = R.f(o, "MaxRotRoll");
            d.MinRotPitch = R.f(o, "MinRotPitch"); d.MaxRotPitch = R.f(o, "MaxRotPitch"); d.MinPScale = R.f(o, "MinPScale");
            d.MaxPScale = R.f(o, "MaxPScale");
            // the payload is unauthenticated: one 64 KiB packet must not be able to ask for gigabytes of instances
            if (d.InstanceCount > XK_WORLD_MAX_INSTANCES_PER_OBJECT && R.err.empty())
                R.err = "InstanceCount of '" + d.ProfabName + "' exceeds " + std::to_string(XK_WORLD_MAX_INSTANCES_PER_OBJECT);
            w.ObjectDescs.push_back(d);
        }
    if (!R.err.empty()) { err = "[WORLD] JSON schema error: " + R.err; return false; }
    if (w.DirectionalLights.size() > XK_MAX_DIRECTIONAL_LIGHTS_NUM || w.PointLights.size() > XK_MAX_POINT_LIGHTS_NUM ||
        w.SpotLights.size() > XK_MAX_SPOT_LIGHTS_NUM) { err = "[WORLD] too many lights (limits 16 / 512 / 16, ZE:84-86)"; return false; }
    w.loaded = true;
    return true;
}

// XkObjectDesc::GenerateInstance, ZE:573-589
void zr_world_generate_instances(const ZrObjectDesc& d, uint64_t seed, std::vector<XkInstanceData>& out)
{
    out.assign(d.InstanceCount, XkInstanceData());
    Pcg32 g(seed);
    for (uint32_t i = 0; i < d.InstanceCount; ++i) {
        XkInstanceData& I = out[i]; memset(&I, 0, sizeof I);
        const float deg = g.range(0.0f, 360.0f);
        const float dist = g.range(d.MinRadius, d.MaxRadius);
        const float rad = deg * 0.01745329251994329576923690768489f;
        I.InstancePosition[0] = sinf(rad) * dist; I.InstancePosition[1] = cosf(rad) * dist; I.InstancePosition[2] = 0.0f;
        I.InstanceRotation[0] = 0.0f; I.InstanceRotation[1] = 3.14159265358979323846f * g.range(0.0f, 180.0f); I.InstanceRotation[2] = 0.0f;
        I.InstancePScale = g.range(d.MinPScale, d.MaxPScale);
        I.InstanceTexIndex = (uint8_t)(g.next() >> 24);
    }
}

bool zr_world_same_cube_names(const ZrWorld& a, const ZrWorld& b)
{
    for (int i = 0; i < 6; ++i) if (a.CubemapFileNames[i] != b.CubemapFileNames[i]) return false;
    return true;
}

// ZR_WORLD_DIFF_*: which parts of two parsed worlds differ (values compared as the bits the parser made of them)
uint32_t zr_world_diff(const ZrWorld& a, const ZrWorld& b)
{
    uint32_t d = 0;
    if (memcmp(&a.MainCamera, &b.MainCamera, sizeof(zr_camera)) != 0) d |= ZR_WORLD_DIFF_CAMERA;
    if (!same_lights(a.DirectionalLights, b.DirectionalLights) || !same_lights(a.PointLights, b.PointLights) || !same_lights(a.SpotLights, b.SpotLights))
        d |= ZR_WORLD_DIFF_LIGHTS;
    if (a.EnableSkydome != b.EnableSkydome || a.OverrideSkydome != b.OverrideSkydome || a.SkydomeFileName != b.SkydomeFileName ||
        a.OverrideCubemap != b.OverrideCubemap || !zr_world_same_cube_names(a, b)) d |= ZR_WORLD_DIFF_SKY;
    if (a.EnableBackground != b.EnableBackground || a.OverrideBackground != b.OverrideBackground || a.BackgroundFileName != b.BackgroundFileName)
        d |= ZR_WORLD_DIFF_BACKGROUND;
    bool objs = a.ObjectDescs.size() == b.ObjectDescs.size();
    for (size_t i = 0; objs && i < a.ObjectDescs.size(); ++i) objs = same_desc(a.ObjectDescs[i], b.ObjectDescs[i]);
    if (!objs) d |= ZR_WORLD_DIFF_OBJECTS;
    return d;
}

// XkWorld::Save (ZE:1149-1263), PrettyWriter layout (4-space indent).  The engine writes OverrideCubemap from
// EnableSkydome (ZE:1175); that bug is NOT reproduced, so Load(Save(w)) == w - for a world whose floats are finite: a number beyond the
// range of a float (1e39) parses to an infinity, which is written as "inf" and refused by Load.
std::string zr_world_to_json(const ZrWorld& w)
{
    std::string o;
    auto arr3 = [&](const char* k, const float* v, int n, const char* ind) {
        o += ind; o += "\""; o += k; o += "\": [\n";
        for (int i = 0; i < n; ++i) { o += ind; o += "    "; jnum(o, v[i]); o += (i + 1 < n) ? ",\n" : "\n"; }
        o += ind; o += "]";
    };
    o += "{\n    \"MainCamera\": {\n";
    arr3("Position", w.MainCamera.Position, 3, "        "); o += ",\n";
    arr3("Lookat", w.MainCamera.Lookat, 3, "        "); o += ",\n";
    o += "        \"Speed\": "; jnum(o, w.MainCamera.Speed); o += ",\n        \"FOV\": "; jnum(o, w.MainCamera.FOV);
    o += ",\n        \"zNear\": "; jnum(o, w.MainCamera.zNear); o += ",\n        \"zFar\": "; jnum(o, w.MainCamera.zFar); o += "\n    },\n";
    o += "    \"Skydome\": {\n        \"EnableSkydome\": "; o += w.EnableSkydome ? "true" : "false";
    o += ",\n        \"OverrideSkydome\": "; o += w.OverrideSkydome ? "true" : "false";
    o += ",\n        \"SkydomeFileName\": "; jstr(o, w.SkydomeFileName);
    o += ",\n        \"OverrideCubemap\": "; o += w.OverrideCubemap ? "true" : "false";
    o += ",\n        \"CubemapFileNames\": [\n";
    for (int i = 0; i < 6; ++i) { o += "            "; jstr(o, w.CubemapFileNames[i]); o += i < 5 ? ",\n" : "\n"; }
    o += "        ]\n    },\n";
    o += "    \"Background\": {\n        \"EnableBackground\": "; o += w.EnableBackground ? "true" : "false";
    o += ",\n        \"OverrideBackground\": "; o += w.OverrideBackground ? "true" : "false";
    o += ",\n        \"BackgroundFileName\": "; jstr(o, w.BackgroundFileName); o += "\n    },\n";
    auto lights = [&](const char* key, const std::vector<ZrLightDesc>& ls) {
        o += "    \""; o += key; o += "\": [";
        for (size_t i = 0; i < ls.size(); ++i) {
            const ZrLightDesc& l = ls[i];
            o += i ? ",\n        {\n" : "\n        {\n";
            arr3("Position", l.Position, 3, "            "); o += ",\n            \"Type\": " + std::to_string(l.Type) + ",\n";
            arr3("Color", l.Color, 3, "            "); o += ",\n            \"Intensity\": "; jnum(o, l.Intensity); o += ",\n";
            arr3("Direction", l.Direction, 3, "            "); o += ",\n            \"Radius\": "; jnum(o, l.Radius); o += ",\n";
            arr3("ExtraData", l.ExtraData, 4, "            "); o += "\n        }";
        }
        o += ls.empty() ? "],\n" : "\n    ],\n";
    };
    lights("DirectionalLights", w.DirectionalLights); lights("PointLights", w.PointLights); lights("SpotLights", w.SpotLights);
    o += "    \"Objects\": [";
    for (size_t i = 0; i < w.ObjectDescs.size(); ++i) {
        const ZrObjectDesc& d = w.ObjectDescs[i];
        o += i ? ",\n        {\n" : "\n        {\n";
        o += "            \"RenderFlags\": " + std::to_string(d.RenderFlags & 0xFFFFu) + ",\n            \"ProfabName\": "; jstr(o, d.ProfabName);
        o += ",\n            \"InstanceCount\": " + std::to_string(d.InstanceCount);
        const char* keys[10] = { "MinRadius", "MaxRadius", "MinRotYaw", "MaxRotYaw", "MinRotRoll", "MaxRotRoll", "MinRotPitch", "MaxRotPitch", "MinPScale", "MaxPScale" };
        const float vals[10] = { d.MinRadius, d.MaxRadius, d.MinRotYaw, d.MaxRotYaw, d.MinRotRoll, d.MaxRotRoll, d.MinRotPitch, d.MaxRotPitch, d.MinPScale, d.MaxPScale };
        for (int k = 0; k < 10; ++k) { o += ",\n            \""; o += keys[k]; o += "\": "; jnum(o, vals[k]); }
        o += "\n        }";
    }
    o += w.ObjectDescs.empty() ? "]\n}" : "\n    ]\n}";
    return o;
}
