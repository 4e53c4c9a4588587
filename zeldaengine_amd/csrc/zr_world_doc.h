// zr_world_doc.h — the world document: XkWorld (ZE:1025-1291) as parsed from JSON, and what reads, writes and compares it
// (zr_world_doc.cpp).  Plain C++17, nothing of HIP: the payload is an outsider's bytes, and tests/host_readers_check.cpp runs this code
// alone on the CPU, under the sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zelda_render.h"

struct ZrLightDesc { float Position[3]; uint32_t Type; float Color[3]; float Intensity; float Direction[3]; float Radius; float ExtraData[4]; };
struct ZrObjectDesc {
    uint32_t RenderFlags = 0; std::string ProfabName; uint32_t InstanceCount = 0;
    float MinRadius = 0, MaxRadius = 0, MinRotYaw = 0, MaxRotYaw = 0, MinRotRoll = 0, MaxRotRoll = 0,
          MinRotPitch = 0, MaxRotPitch = 0, MinPScale = 0, MaxPScale = 0;
};
struct ZrWorld {
    bool EnableSkydome = true, OverrideSkydome = false; std::string SkydomeFileName;
    bool OverrideCubemap = false; std::string CubemapFileNames[6];
    bool EnableBackground = false, OverrideBackground = false; std::string BackgroundFileName;
    zr_camera MainCamera;
    std::vector<ZrLightDesc> DirectionalLights, PointLights, SpotLights;
    std::vector<ZrObjectDesc> ObjectDescs;
    bool loaded = false;
};

// XkWorld::Load, ZE:1051-1147: `w` reset, then read from the len bytes at utf8.  Returns false with `err` set on a parse or schema error.
bool zr_world_parse(const char* utf8, size_t len, ZrWorld& w, std::string& err);
// XkWorld::Save (ZE:1149-1263), PrettyWriter layout
std::string zr_world_to_json(const ZrWorld& w);
// ZR_WORLD_DIFF_*: which parts of two parsed worlds differ (values compared as the bits the parser made of them)
uint32_t zr_world_diff(const ZrWorld& a, const ZrWorld& b);
bool zr_world_same_cube_names(const ZrWorld& a, const ZrWorld& b);
// XkObjectDesc::GenerateInstance, ZE:573-589: the d.InstanceCount instances of one object
void zr_world_generate_instances(const ZrObjectDesc& d, uint64_t seed, std::vector<XkInstanceData>& out);
