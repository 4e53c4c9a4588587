// zelda_headless — a native caller of the C-ABI: the engine's main loop without a window.
//
// Replaces XkZeldaEngineApp::Run / MainTick / DrawFrame (ZE:1576, 1743, 1940) for a host that has no Vulkan surface: create the
// renderer, point it at the engine's content tree, load a world (file, or wait for one over the livelink), then per frame
//     zr_livelink_poll (bReloadScene pickup, ZE:1943-1951) -> zr_world_update_uniforms (UpdateWorld + UpdateUniformBuffer) -> zr_render
// and finally write the last frame as a PPM.  Uses nothing but include/zelda_render.h; links -lzelda_render.
//
//   zelda_headless --root DIR [--world FILE.json] [--livelink PORT [--wait-ms MS]] [--meshlet FILE.meshlet --profab NAME]
//                  [--size WxH] [--shadow N] [--frames N] [--roll-light-step F] [--debug-view V] [--out FRAME.ppm] [--device D]
//                  [--pick X,Y[,W,H] [--highlight]] [--incremental] [--delta | --delta-packed] [--scale S] [--resize-at FRAME:WxH]
//                  [--overlay FILE] [--overlay-box] [--raycast X,Y] [--wire[=WIDTH_256]] [--wire-selected]
// --resize-at FRAME:WxH gives the live context a new extent ahead of frame FRAME (zr_resize), as a host whose window changes size does:
// nothing is loaded again, it prints `resized <W>x<H>`, and with --delta, --delta-packed or --scale the client copy and the delivery
// buffers follow the new (scaled) extent - the next delivery is a full one.
// --incremental applies livelink payloads as a difference from the live scene (zr_livelink_set_incremental): a payload that only moves
// the camera or a light keeps every object, the visibility history and the shadow map.
// --delta delivers every frame the way a host with a remote client does (zr_read_frame_delta): only the 32 x 32 tiles that differ from
// what was delivered last leave the GPU and are applied to a client copy of the frame; it prints `delta <tiles>/<total>` per frame, and
// --out is written from the client copy.
// --delta-packed does the same through the compressed form (zr_read_frame_delta_packed): the listed tiles leave the GPU as records of the
// tile codec and zr_frame_delta_decode applies them to the client copy; it prints `delta-packed <tiles>/<total> tiles <bytes> bytes (<raw> raw)`.
// --scale S (1..8) delivers the frame box-filtered by S in linear light (zelda_render.h, "delivering a scaled frame"): with --delta or
// --delta-packed it is the delta scale (zr_set_frame_delta_scale) and the client copy has the scaled extent; without them every frame is
// read with zr_read_color_scaled and it prints `scaled <Wd>x<Hd>` per frame.  --out writes the client copy at the scaled extent.
// --pick keeps the last frame's per-pixel winners (zr_set_id_capture) and prints what zr_pick finds in the rectangle (default 1 x 1),
// one JSON line per hit, nearest first - what an editor does on a click.
// --raycast X,Y casts the camera's ray through the centre of pixel (X, Y) into the scene of the last frame (zr_camera_ray at X + 0.5,
// Y + 0.5, then zr_raycast; no id capture needed) and prints the hit as one JSON line in --pick's format plus t, the weights, the world
// position and the face normal - `{"hit": 0}` for a miss.
// --highlight (with --pick) shows the selection: the pick is made after the first frame, its hits go into the highlight set
// (zr_highlight_set) and every following frame is delivered highlighted (zelda_render.h, "highlighting a selection") through whichever of
// --delta, --delta-packed and --scale is chosen - zr_set_frame_delta_highlight, or zr_read_color_highlighted at the scale, which prints
// `highlighted <Wd>x<Hd>` per frame.  --out writes the highlighted picture.
// --overlay FILE draws line segments over every delivered frame (zelda_render.h, "overlaying lines"): FILE holds one segment per line,
// `ax ay az bx by bz r g b a flags` (blank lines and lines that start with # are skipped); the list is set once (zr_overlay_set) and
// every frame is delivered overlaid through whichever of --delta, --delta-packed, --scale and --highlight is chosen -
// zr_set_frame_delta_overlay, or zr_read_color_overlaid at the scale, which prints `overlaid <Wd>x<Hd>` per frame.  --out writes the
// overlaid picture.
// --wire[=WIDTH_256] draws the visible triangles' edges over every delivered frame (zelda_render.h, "wireframe"; opaque black, WIDTH_256
// in 1/256 pixel, default 256), first of the stages: through zr_set_frame_delta_wire with --delta, else zr_read_color_staged at the scale
// with whatever --highlight and --overlay add, which prints `wired <Wd>x<Hd>` per frame.  --wire-selected (with --pick X,Y --highlight)
// draws it on the picked instances only (ZR_WIRE_SELECTED).  --out writes the wired picture.
// --overlay-box (with --pick) draws the twelve edges of each picked instance's bounds: the pick is made after the first frame, the box
// of the mesh's vertices (zr_mesh_get_vertices) is taken through the instance's scale, rotation and position (zr_object_get_instances:
// the vertex stage's own transform, in double precision) and its edges join the list - yellow, hidden parts at a third - so every
// following frame shows them; it prints `overlay-box <object> <instance>` per box.
#include "../include/zelda_render.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

static int fail(zr_ctx* c, const char* what, int rc)
{
    fprintf(stderr, "zelda_headless: %s failed (%d): %s\n", what, rc, zr_last_error(c));
    if (c) zr_destroy(c);
    return 1;
}

int main(int argc, char** argv)
{
    std::string root = ".", world, meshlet, profab = "meshlet", out, overlay;
    uint32_t W = 1920, H = 1080, SD = 1024, frames = 1, debug_view = 0, scale = 0;
    int port = -1, wait_ms = 10000, device = 0;
    float roll_step = 0.0f;
    bool pick = false, incremental = false, delta = false, packed = false, highlight = false, overlay_box = false; uint32_t px = 0, py = 0, pw = 1, ph = 1;
    uint32_t resize_at = 0xFFFFFFFFu, RW = 0, RH = 0;
    bool raycast = false; uint32_t rx = 0, ry = 0;
    bool wire = false, wire_selected = false; uint32_t wire_width = 256;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a.c_str()); exit(2); } return argv[++i]; };
        if (a == "--root") root = next();
        else if (a == "--world") world = next();
        else if (a == "--meshlet") meshlet = next();
        else if (a == "--profab") profab = next();
        else if (a == "--out") out = next();
        else if (a == "--size") { if (sscanf(next(), "%ux%u", &W, &H) != 2) { fprintf(stderr, "--size WxH\n"); return 2; } }
        else if (a == "--shadow") SD = (uint32_t)atoi(next());
        else if (a == "--frames") frames = (uint32_t)atoi(next());
        else if (a == "--debug-view") debug_view = (uint32_t)atoi(next());
        else if (a == "--livelink") port = atoi(next());
        else if (a == "--wait-ms") wait_ms = atoi(next());
        else if (a == "--device") device = atoi(next());
        else if (a == "--roll-light-step") roll_step = (float)atof(next());
        else if (a == "--incremental") incremental = true;
        else if (a == "--delta") delta = true;
        else if (a == "--delta-packed") delta = packed = true;
        else if (a == "--scale") scale = (uint32_t)atoi(next());
        else if (a == "--highlight") highlight = true;
        else if (a == "--overlay") overlay = next();
        else if (a == "--overlay-box") overlay_box = true;
        else if (a == "--wire") wire = true;
        else if (a.rfind("--wire=", 0) == 0) { wire = true; wire_width = (uint32_t)atoi(a.c_str() + 7); }
        else if (a == "--wire-selected") wire = wire_selected = true;
        else if (a == "--resize-at") { if (sscanf(next(), "%u:%ux%u", &resize_at, &RW, &RH) != 3) { fprintf(stderr, "--resize-at FRAME:WxH\n"); return 2; } }
        else if (a == "--pick") {
            const int got = sscanf(next(), "%u,%u,%u,%u", &px, &py, &pw, &ph);
            if (got != 2 && got != 4) { fprintf(stderr, "--pick X,Y[,W,H]\n"); return 2; }
            pick = true;
        }
        else if (a == "--raycast") { if (sscanf(next(), "%u,%u", &rx, &ry) != 2) { fprintf(stderr, "--raycast X,Y\n"); return 2; } raycast = true; }
        else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (highlight && !pick) { fprintf(stderr, "--highlight needs --pick X,Y[,W,H]\n"); return 2; }
    if (overlay_box && !pick) { fprintf(stderr, "--overlay-box needs --pick X,Y[,W,H]\n"); return 2; }
    if (wire_selected && !highlight) { fprintf(stderr, "--wire-selected needs --pick X,Y[,W,H] --highlight\n"); return 2; }
    zr_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.width = W; cfg.height = H; cfg.shadow_dim = SD; cfg.debug_view = debug_view; cfg.device = device; cfg.tile_world = 1;
    zr_ctx* c = nullptr;
    int rc = zr_create(&cfg, &c);
    if (rc) { fprintf(stderr, "zelda_headless: zr_create failed (%d): no usable HIP device? (there is no CPU fallback)\n", rc); return 1; }
    if ((rc = zr_set_asset_root(c, root.c_str()))) return fail(c, "zr_set_asset_root", rc);
    if (!meshlet.empty()) {          // the XkMeshIndirect path: a .meshlet file written by the ZeldaMeshlet tool, registered as a Profab
        uint32_t mesh = 0;
        if ((rc = zr_load_meshlet_file(c, meshlet.c_str(), &mesh))) return fail(c, "zr_load_meshlet_file", rc);
        if ((rc = zr_profab_register(c, profab.c_str(), mesh, nullptr))) return fail(c, "zr_profab_register", rc);
    }
    bool have_world = false;
    if (!world.empty()) {
        if ((rc = zr_world_load_file(c, world.c_str()))) return fail(c, "zr_world_load_file", rc);
        have_world = true;
    }
    if (incremental && (rc = zr_livelink_set_incremental(c, 1))) return fail(c, "zr_livelink_set_incremental", rc);
    if (port >= 0) {
        if ((rc = zr_livelink_serve(c, (uint16_t)port))) return fail(c, "zr_livelink_serve", rc);
        uint16_t p = 0; zr_livelink_port(c, &p);
        printf("[Socket] listening on port %u\n", (unsigned)p); fflush(stdout);
        for (int waited = 0; !have_world && waited < wait_ms; waited += 10) {
            int reloaded = 0;
            if ((rc = zr_livelink_poll(c, &reloaded))) return fail(c, "zr_livelink_poll", rc);
            if (reloaded) have_world = true; else std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
    }
    if (!have_world) { fprintf(stderr, "zelda_headless: no world (give --world FILE or send one to --livelink PORT)\n"); zr_destroy(c); return 1; }

    if ((pick || wire) && (rc = zr_set_id_capture(c, 1))) return fail(c, "zr_set_id_capture", rc);
    if (wire) {
        const zr_wire_style st = { { 0, 0, 0, 255 }, wire_width, wire_selected ? ZR_WIRE_SELECTED : 0u, 0u };
        if ((rc = zr_set_wire_style(c, &st, sizeof st))) return fail(c, "zr_set_wire_style (--wire=1..4096)", rc);
    }
    std::vector<zr_overlay_segment> segs;
    if (!overlay.empty()) {          // --overlay: the list, read once
        FILE* fp = fopen(overlay.c_str(), "r");
        if (!fp) { fprintf(stderr, "zelda_headless: cannot read %s\n", overlay.c_str()); zr_destroy(c); return 1; }
        char line[512];
        for (unsigned ln = 1; fgets(line, sizeof line, fp); ++ln) {
            const char* p = line + strspn(line, " \t\r\n");
            if (!*p || *p == '#') continue;
            zr_overlay_segment s; unsigned col[4], flags = 0;
            if (sscanf(p, "%f %f %f %f %f %f %u %u %u %u %u", &s.a[0], &s.a[1], &s.a[2], &s.b[0], &s.b[1], &s.b[2], &col[0], &col[1], &col[2], &col[3], &flags) != 11 ||
                col[0] > 255 || col[1] > 255 || col[2] > 255 || col[3] > 255) {
                fprintf(stderr, "zelda_headless: %s:%u: ax ay az bx by bz r g b a flags\n", overlay.c_str(), ln); fclose(fp); zr_destroy(c); return 2;
            }
            for (int k = 0; k < 4; ++k) s.rgba[k] = (uint8_t)col[k];
            s.flags = flags;
            segs.push_back(s);
        }
        fclose(fp);
        if ((rc = zr_overlay_set(c, segs.data(), (uint32_t)segs.size()))) return fail(c, "zr_overlay_set", rc);
    }
    const bool lines = !overlay.empty() || overlay_box;
    if (overlay_box) {
        const zr_overlay_style st = { 0.0f, 85u, { 0u, 0u } };
        if ((rc = zr_set_overlay_style(c, &st, sizeof st))) return fail(c, "zr_set_overlay_style", rc);
    }
    // --overlay-box: the twelve edges of one instance's bounds appended to the list
    auto add_box = [&](uint32_t object, uint32_t instance) -> int {
        uint32_t mesh = 0, n_inst = 0, n_v = 0;
        if ((rc = zr_object_get_instances(c, object, &mesh, nullptr, &n_inst))) return rc;
        std::vector<XkInstanceData> inst(n_inst);
        if (n_inst && (rc = zr_object_get_instances(c, object, &mesh, inst.data(), &n_inst))) return rc;
        if ((rc = zr_mesh_get_vertices(c, mesh, nullptr, &n_v))) return rc;
        std::vector<XkVertex> v(n_v);
        if (!n_v || (rc = zr_mesh_get_vertices(c, mesh, v.data(), &n_v))) return rc;
        double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
        for (const XkVertex& x : v) for (int k = 0; k < 3; ++k) { lo[k] = std::fmin(lo[k], x.Position[k]); hi[k] = std::fmax(hi[k], x.Position[k]); }
        // the vertex stage's instance transform: (p * scale) as a row vector times rotMat = mz * my * mx (column-major), plus the position
        double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, t[3] = { 0, 0, 0 }, sc = 1.0;
        if (instance < n_inst) {
            const XkInstanceData& I = inst[instance];
            const double ax = I.InstanceRotation[0], ay = I.InstanceRotation[1], az = I.InstanceRotation[2];      // (double: std::cos of a float is cosf)
            const double cx = std::cos(ax), sx = std::sin(ax), cy = std::cos(ay), sy = std::sin(ay), cz = std::cos(az), sz = std::sin(az);
            const double mx[9] = { cx, 0, sx, 0, 1, 0, -sx, 0, cx }, my[9] = { cy, sy, 0, -sy, cy, 0, 0, 0, 1 }, mz[9] = { 1, 0, 0, 0, cz, sz, 0, -sz, cz };
            double zy[9];
            auto mul = [](const double* A, const double* B, double* C) {
                for (int cc = 0; cc < 3; ++cc) for (int r = 0; r < 3; ++r) C[cc * 3 + r] = A[r] * B[cc * 3] + A[3 + r] * B[cc * 3 + 1] + A[6 + r] * B[cc * 3 + 2];
            };
            mul(mz, my, zy); mul(zy, mx, R);
            sc = I.InstancePScale;
            for (int k = 0; k < 3; ++k) t[k] = I.InstancePosition[k];
        }
        float corner[8][3];
        for (int i = 0; i < 8; ++i) {
            const double p[3] = { ((i & 1) ? hi[0] : lo[0]) * sc, ((i & 2) ? hi[1] : lo[1]) * sc, ((i & 4) ? hi[2] : lo[2]) * sc };
            for (int j = 0; j < 3; ++j) corner[i][j] = (float)(p[0] * R[j * 3] + p[1] * R[j * 3 + 1] + p[2] * R[j * 3 + 2] + t[j]);
        }
        for (int i = 0; i < 8; ++i)
            for (int b = 1; b < 8; b <<= 1) {
                if (i & b) continue;
                zr_overlay_segment s; memset(&s, 0, sizeof s);
                memcpy(s.a, corner[i], sizeof s.a); memcpy(s.b, corner[i | b], sizeof s.b);
                s.rgba[0] = 255; s.rgba[1] = 220; s.rgba[2] = 0; s.rgba[3] = 255;
                segs.push_back(s);
            }
        printf("overlay-box %u %u\n", object, instance);
        return zr_overlay_set(c, segs.data(), (uint32_t)segs.size());
    };
    // --delta: the client's copy of the frame, and full-sized buffers for a delivery (only the listed tiles are written and moved)
    // DW x DH: what is delivered - the frame, or with --scale the scaled one (with --delta: the delta scale's extent, in `total` tiles)
    uint32_t DW = W, DH = H, total = 0, delta_scale = 1;
    const uint32_t scaled = delta ? 0u : scale;           // without --delta: the scale every frame is read at (0: frames are not read)
    std::vector<uint8_t> client, slots; std::vector<uint32_t> list, offsets;
    if (scale && (rc = zr_frame_scaled_extent(W, H, scale, &DW, &DH))) return fail(c, "zr_frame_scaled_extent (--scale 1..8)", rc);
    if (scaled || ((highlight || lines || wire) && !delta)) client.assign((size_t)DW * DH * 4, 0);
    if (wire && delta && (rc = zr_set_frame_delta_wire(c, 1))) return fail(c, "zr_set_frame_delta_wire", rc);
    if (lines && delta && (rc = zr_set_frame_delta_overlay(c, 1))) return fail(c, "zr_set_frame_delta_overlay", rc);
    if (highlight && delta && (rc = zr_set_frame_delta_highlight(c, 1))) return fail(c, "zr_set_frame_delta_highlight", rc);
    if (scale && delta && (rc = zr_set_frame_delta_scale(c, scale))) return fail(c, "zr_set_frame_delta_scale", rc);
    if (delta && (rc = zr_get_frame_delta_extent(c, &DW, &DH, &total, &delta_scale))) return fail(c, "zr_get_frame_delta_extent", rc);
    const uint32_t T = ZR_TILE; uint32_t tiles_x = (DW + T - 1) / T;
    auto size_delivery = [&]() {        // the client copy and a delivery's buffers for DW x DH in `total` tiles
        client.assign((size_t)DW * DH * 4, 0); slots.resize((size_t)total * (packed ? ZR_FRAME_DELTA_RECORD_MAX : T * T * 4)); list.resize(total);
        offsets.resize((size_t)total + 1);
    };
    if (delta) {
        size_delivery();
        if ((rc = zr_set_frame_delta(c, packed ? ZR_FRAME_DELTA_PACKED : 1))) return fail(c, "zr_set_frame_delta", rc);
    }
    // --pick: what zr_pick finds in the rectangle, printed; with --highlight the hits go into the highlight set
    auto do_pick = [&]() -> int {
        uint32_t n = 0;
        if ((rc = zr_pick(c, px, py, pw, ph, nullptr, 0, &n))) return rc;
        std::vector<zr_hit> hits(n);
        if (n && (rc = zr_pick(c, px, py, pw, ph, hits.data(), n, &n))) return rc;
        for (const zr_hit& h : hits) {
            printf("{\"object\": %u, \"instance\": %u, \"pixels\": %u, \"triangle\": %u, \"x\": %u, \"y\": %u, \"depth\": %.9g}\n",
                   h.object, h.instance, h.pixels, h.triangle, h.x, h.y, (double)h.depth);
            const uint8_t on = 1;
            if (highlight && (rc = zr_highlight_set(c, h.object, h.instance, &on, 1))) return rc;
            if (overlay_box && (rc = add_box(h.object, h.instance))) return rc;
        }
        return 0;
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t f = 0; f < frames; ++f) {
        int reloaded = 0;
        if (f == resize_at) {           // the window changed size: a new extent, the same scene (delta state, selection and history of the map stay)
            if ((rc = zr_resize(c, RW, RH)) || (rc = zr_get_extent(c, &W, &H))) return fail(c, "zr_resize", rc);
            DW = W; DH = H;
            if (scale && (rc = zr_frame_scaled_extent(W, H, scale, &DW, &DH))) return fail(c, "zr_frame_scaled_extent", rc);
            if (delta && (rc = zr_get_frame_delta_extent(c, &DW, &DH, &total, &delta_scale))) return fail(c, "zr_get_frame_delta_extent", rc);
            tiles_x = (DW + T - 1) / T;
            if (delta) size_delivery();
            else if (!client.empty()) client.assign((size_t)DW * DH * 4, 0);
            printf("resized %ux%u\n", W, H);
        }
        if (port >= 0 && (rc = zr_livelink_poll(c, &reloaded))) return fail(c, "zr_livelink_poll", rc);
        if ((rc = zr_world_update_uniforms(c, 0.0f, roll_step * (float)f, 0.016f * (float)f))) return fail(c, "zr_world_update_uniforms", rc);
        if ((rc = zr_render(c))) return fail(c, "zr_render", rc);
        if ((highlight || overlay_box) && f == 0 && do_pick()) return fail(c, "zr_pick / zr_highlight_set / zr_overlay_set", rc);      // the click: from here on the selection shows
        if (!delta && wire) {                             // the wired frame, with whatever --highlight and --overlay add, at the scale
            const uint32_t stages = ZR_STAGE_WIRE | (highlight ? ZR_STAGE_HIGHLIGHT : 0u) | (lines ? ZR_STAGE_OVERLAY : 0u);
            if ((rc = zr_read_color_staged(c, stages, scale ? scale : 1u, client.data(), client.size()))) return fail(c, "zr_read_color_staged", rc);
            printf("wired %ux%u\n", DW, DH);
        }
        else if (!delta && lines) {                       // the overlaid frame (highlighted underneath or not), at the scale
            if ((rc = zr_read_color_overlaid(c, scale ? scale : 1u, highlight ? 1 : 0, client.data(), client.size()))) return fail(c, "zr_read_color_overlaid", rc);
            printf("overlaid %ux%u\n", DW, DH);
        }
        else if (!delta && highlight) {                   // the highlighted frame, at the scale, is all that crosses the link
            if ((rc = zr_read_color_highlighted(c, scale ? scale : 1u, client.data(), client.size()))) return fail(c, "zr_read_color_highlighted", rc);
            printf("highlighted %ux%u\n", DW, DH);
        }
        else if (!delta && scaled) {                           // the scaled frame is all that crosses the link
            if ((rc = zr_read_color_scaled(c, scaled, client.data(), client.size()))) return fail(c, "zr_read_color_scaled", rc);
            printf("scaled %ux%u\n", DW, DH);
        }
        if (!delta) continue;
        if (packed) {                                     // the records cross the link; the client's side is the library's decoder
            zr_frame_delta_packed d;
            if ((rc = zr_read_frame_delta_packed(c, list.data(), total, offsets.data(), total + 1, slots.data(), slots.size(), &d, sizeof d)))
                return fail(c, "zr_read_frame_delta_packed", rc);
            if ((rc = zr_frame_delta_decode(list.data(), offsets.data(), d.n_tiles, slots.data(), d.bytes, DW, DH, client.data())))
                return fail(c, "zr_frame_delta_decode", rc);
            printf("delta-packed %u/%u tiles %u bytes (%u raw)\n", d.n_tiles, d.total_tiles, d.bytes, d.raw_tiles);
            continue;
        }
        zr_frame_delta d;
        if ((rc = zr_read_frame_delta(c, list.data(), total, slots.data(), slots.size(), &d, sizeof d))) return fail(c, "zr_read_frame_delta", rc);
        for (uint32_t k = 0; k < d.n_tiles; ++k) {        // the client's apply loop: the rows of each listed tile that lie inside the frame
            const uint32_t x0 = list[k] % tiles_x * T, y0 = list[k] / tiles_x * T, w = DW - x0 < T ? DW - x0 : T, h = DH - y0 < T ? DH - y0 : T;
            for (uint32_t y = 0; y < h; ++y)
                memcpy(&client[((size_t)(y0 + y) * DW + x0) * 4], &slots[((size_t)k * T + y) * T * 4], (size_t)w * 4);
        }
        printf("delta %u/%u\n", d.n_tiles, d.total_tiles);
    }
    if ((rc = zr_finish(c))) return fail(c, "zr_finish", rc);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    zr_stats st;
    if ((rc = zr_get_stats(c, &st, sizeof st))) return fail(c, "zr_get_stats", rc);
    uint32_t n_obj = 0; zr_object_count(c, &n_obj);
    printf("frames %u  %.3f ms/frame  objects %u  meshlet-instances %llu  camera survivors %llu  covered pixels %llu\n", frames, ms / frames, n_obj,
           (unsigned long long)st.work_items[1], (unsigned long long)st.survivors[1], (unsigned long long)st.covered_pixels);
    if (pick && !highlight && !overlay_box && do_pick()) return fail(c, "zr_pick", rc);
    if (raycast) {                                        // the camera's ray through the pixel's centre, into the scene of the last frame
        zr_ray ray; zr_ray_hit h;
        if ((rc = zr_camera_ray(c, (float)rx + 0.5f, (float)ry + 0.5f, &ray))) return fail(c, "zr_camera_ray", rc);
        if ((rc = zr_raycast(c, &ray, 1u, 0u, &h, sizeof h))) return fail(c, "zr_raycast", rc);
        if (!(h.flags & ZR_RAY_HIT)) printf("{\"hit\": 0, \"x\": %u, \"y\": %u}\n", rx, ry);
        else
            printf("{\"hit\": 1, \"object\": %u, \"instance\": %u, \"triangle\": %u, \"x\": %u, \"y\": %u, \"back\": %u, \"t\": %.9g, \"u\": %.9g, \"v\": %.9g, "
                   "\"position\": [%.9g, %.9g, %.9g], \"normal\": [%.9g, %.9g, %.9g]}\n",
                   h.object, h.instance, h.triangle, rx, ry, (h.flags & ZR_RAY_HIT_BACK) ? 1u : 0u, (double)h.t, (double)h.u, (double)h.v,
                   (double)ray.origin[0] + (double)h.t * (double)ray.dir[0], (double)ray.origin[1] + (double)h.t * (double)ray.dir[1],
                   (double)ray.origin[2] + (double)h.t * (double)ray.dir[2], (double)h.normal[0], (double)h.normal[1], (double)h.normal[2]);
    }
    if (!out.empty()) {
        std::vector<uint8_t> rgba((size_t)DW * DH * 4);
        if (delta || scaled || highlight || lines || wire) rgba = client;
        else if ((rc = zr_read_color(c, rgba.data(), rgba.size()))) return fail(c, "zr_read_color", rc);
        FILE* fp = fopen(out.c_str(), "wb");
        if (!fp) { fprintf(stderr, "zelda_headless: cannot write %s\n", out.c_str()); zr_destroy(c); return 1; }
        fprintf(fp, "P6\n%u %u\n255\n", DW, DH);
        std::vector<uint8_t> rgb((size_t)DW * DH * 3);
        for (size_t i = 0; i < (size_t)DW * DH; ++i) { rgb[3 * i] = rgba[4 * i]; rgb[3 * i + 1] = rgba[4 * i + 1]; rgb[3 * i + 2] = rgba[4 * i + 2]; }
        fwrite(rgb.data(), 1, rgb.size(), fp);
        fclose(fp);
    }
    zr_destroy(c);
    return 0;
}
