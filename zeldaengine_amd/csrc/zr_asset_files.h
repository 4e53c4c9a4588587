// zr_asset_files.h — the readers of OBJ and PNG files (zr_asset_files.cpp).  Plain C++17, nothing of HIP: a world payload names these
// files, and tests/host_readers_check.cpp runs the readers alone on the CPU, under the sanitizers.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zelda_abi.h"

// Names that arrive in a (possibly unauthenticated) world payload must stay inside the content tree: no absolute path, no ".."
// component, no NUL.
bool zr_payload_name_ok(const std::string& name);
// LoadMeshAsset (OBJ branch), ZE:6899-6948: vertices deduplicated on the whole record, three indices per triangle.  false with `err` set.
bool zr_obj_ingest(const std::string& path, std::vector<XkVertex>* v, std::vector<uint32_t>* idx, std::string* err);
// stbi_load(path, &w, &h, &n, STBI_rgb_alpha) for PNG files: W * H * 4 bytes of RGBA8, at most 16 384 on a side.  false with `err` set.
bool zr_png_load(const std::string& path, std::vector<uint8_t>* rgba, uint32_t* W, uint32_t* H, std::string* err);
