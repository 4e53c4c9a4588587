// zr_world.cpp — a world instantiated, and applied as a difference; the Profab registry; the world entry points of the C-ABI.
//
// Replaces the scene-building half of CreateEngineScene (ZE:4250-4267).  The document itself - XkWorld::Load / Save / Reset - is
// zr_world_doc.cpp (plain C++), the socket listener zr_livelink.cpp.
#include "zr_ctx.h"

#include <algorithm>
#include <cstring>
#include <new>

namespace {

int world_uniforms(zr_ctx* c, const ZrWorld& w, float roll_stage, float roll_light, float time);

// where a world's object came from (the matching rules of zr_world_update_json, include/zelda_render.h)
void world_tag(ZrSceneObject& o, const std::string& profab, uint32_t model)
{
    o.profab = profab; o.profab_model = model; o.from_world = true; o.mat_pristine = true;
}

int apply_world(zr_ctx* c, const ZrWorld& w)
{
    // CreateEngineScene (ZE:4250-4267): drop the render objects, keep meshes and registered Profabs
    int rc = ZR_OK;
    {
        auto keep_m = std::move(c->meshes); auto keep_p = std::move(c->profabs);
        c->objects.clear(); c->scene_dirty = true; c->scene_gen++; zr_casters_changed(c);      // (each object releases its device memory)
        c->meshes = std::move(keep_m); c->profabs = std::move(keep_p);
    }
    c->world = w;
    zr_set_sky_flags(c, w.EnableSkydome ? 1 : 0, w.EnableBackground ? 1 : 0);       // gates of ZE:3682 / ZE:3693
    rc = zr_world_apply_overrides(c, w);            // CreateEngineScene (1): cubemap / skydome / background named by the world, via ASSETS()
    for (size_t oi = 0; oi < w.ObjectDescs.size() && rc == ZR_OK; ++oi) {
        const ZrObjectDesc& d = w.ObjectDescs[oi];
        auto it = c->profabs.find(d.ProfabName);
        if (it == c->profabs.end() && c->assets_on) {          // not registered by the host: look for Profabs/<name> on disk (ZE:4922-5000)
            int found = 0;
            rc = zr_profab_from_disk(c, d.ProfabName, &found);
            if (rc) break;
            it = c->profabs.find(d.ProfabName);
        }
        if (it == c->profabs.end()) continue;      // no such Profab directory: the engine finds no models and draws nothing
        std::vector<XkInstanceData> inst;
        if (d.InstanceCount > 1) zr_world_generate_instances(d, 1234u + oi, inst);
        for (size_t mi = 0; mi < it->second.size(); ++mi) {
            const ZrProfab& pf = it->second[mi];
            rc = zr_object_add_internal(c, pf.mesh, pf.mat, inst.empty() ? nullptr : inst.data(), (uint32_t)inst.size());
            if (rc) break;
            world_tag(c->objects.back(), d.ProfabName, (uint32_t)mi);
        }
    }
    if (rc) return rc;
    if (c->assets_on) {                 // (what zr_world_apply_overrides set is the world's: zr_world_update_json re-reads it only when its name changes)
        if (w.OverrideCubemap) c->world_named[0] = true;
        if (w.OverrideSkydome) c->world_named[1] = true;
        if (w.OverrideBackground) c->world_named[2] = true;
    }
    return world_uniforms(c, w, 0.0f, 0.0f, 0.0f);
}

int world_uniforms(zr_ctx* c, const ZrWorld& w, float roll_stage, float roll_light, float time)
{
    std::vector<XkLight> L[3];
    const std::vector<ZrLightDesc>* src[3] = { &w.DirectionalLights, &w.PointLights, &w.SpotLights };
    for (int k = 0; k < 3; ++k)
        for (const ZrLightDesc& l : *src[k]) {      // XkLight(const XkLightDesc&), ZE:781-787
            XkLight x;
            x.Position[0] = l.Position[0]; x.Position[1] = l.Position[1]; x.Position[2] = l.Position[2]; x.Position[3] = (float)(uint8_t)l.Type;
            x.Color[0] = l.Color[0]; x.Color[1] = l.Color[1]; x.Color[2] = l.Color[2]; x.Color[3] = l.Intensity;
            x.Direction[0] = l.Direction[0]; x.Direction[1] = l.Direction[1]; x.Direction[2] = l.Direction[2]; x.Direction[3] = l.Radius;
            memcpy(x.LightInfo, l.ExtraData, 16);
            L[k].push_back(x);
        }
    return zr_update_uniforms(c, &w.MainCamera, L[0].data(), (uint32_t)L[0].size(), L[1].data(), (uint32_t)L[1].size(),
                              L[2].data(), (uint32_t)L[2].size(), roll_stage, roll_light, time);
}

// ------------------------------------------------------------------------------------------------ a world applied as a difference

// One entry of the target list (what apply_world would build) and what becomes of it: the live object it takes (-1: none, it is added)
struct WorldTarget {
    uint32_t desc, model; int live;
    enum Act { Add, Keep, Reinstance, Resize } act;
    bool rebuild_material, show;
};

// zr_world_update_json behind its parse.  Two phases: the plan reads files, resolves Profabs and matches targets with live objects and
// changes nothing a frame can see; the commit cannot be refused any more (a device failure aside).
int update_world(zr_ctx* c, const ZrWorld& w, zr_world_delta& D)
{
    D.differs = zr_world_diff(c->world, w);
    // ---- plan: cubemap, skydome, background - re-read only under a new name, or when the host replaced what the world had named
    ZrOverridePlan plan;
    if (c->assets_on) {
        const ZrWorld& o = c->world;
        const bool cube_same = c->world_named[0] && o.OverrideCubemap && zr_world_same_cube_names(o, w);
        const bool sky_same = c->world_named[1] && o.OverrideSkydome && o.SkydomeFileName == w.SkydomeFileName;
        const bool bg_same = c->world_named[2] && o.OverrideBackground && o.BackgroundFileName == w.BackgroundFileName;
        if (w.OverrideCubemap) { if (!cube_same) plan.which |= 1u; } else if (c->world_named[0]) plan.clear |= 1u;
        if (w.OverrideSkydome) { if (!sky_same) plan.which |= 2u; } else if (c->world_named[1]) plan.clear |= 2u;
        if (w.OverrideBackground) { if (!bg_same) plan.which |= 4u; } else if (c->world_named[2]) plan.clear |= 4u;
    }
    int rc = zr_world_plan_overrides(c, w, &plan);
    if (rc) return rc;
    // ---- plan: the target list
    std::vector<std::vector<XkInstanceData>> inst(w.ObjectDescs.size());
    std::vector<WorldTarget> T;
    std::vector<char> used(c->objects.size(), 0);
    bool any_reinstance = false, any_show = false, structural = false;
    for (size_t oi = 0; oi < w.ObjectDescs.size(); ++oi) {
        const ZrObjectDesc& d = w.ObjectDescs[oi];
        auto it = c->profabs.find(d.ProfabName);
        if (it == c->profabs.end() && c->assets_on) {          // (read into the Profab cache: nothing a frame sees)
            int found = 0;
            rc = zr_profab_from_disk(c, d.ProfabName, &found);
            if (rc) return rc;
            it = c->profabs.find(d.ProfabName);
        }
        if (it == c->profabs.end()) continue;
        if (d.InstanceCount > 1) zr_world_generate_instances(d, 1234u + oi, inst[oi]);
        const uint32_t want_n = inst[oi].empty() ? 1u : (uint32_t)inst[oi].size();
        for (size_t mi = 0; mi < it->second.size(); ++mi) {
            WorldTarget t = { (uint32_t)oi, (uint32_t)mi, -1, WorldTarget::Add, false, false };
            for (size_t li = 0; li < c->objects.size(); ++li) {
                const ZrSceneObject& o = c->objects[li];
                if (used[li] || !o.from_world || o.profab_model != mi || o.mesh != it->second[mi].mesh || o.profab != d.ProfabName) continue;
                used[li] = 1; t.live = (int)li;
                break;
            }
            if (t.live >= 0) {
                const ZrSceneObject& o = c->objects[(size_t)t.live];
                if (o.instanced != !inst[oi].empty() || o.n_inst != want_n) t.act = WorldTarget::Resize;
                else if (!o.instanced || (!o.host_stale && memcmp(o.inst.data(), inst[oi].data(), sizeof(XkInstanceData) * want_n) == 0)) t.act = WorldTarget::Keep;
                else t.act = WorldTarget::Reinstance;
                t.rebuild_material = !o.mat_pristine;
                t.show = o.hidden || o.vis_stale;
                for (uint8_t v : o.vis) if (!v) t.show = true;
            }
            switch (t.act) {
            case WorldTarget::Add: D.objects_added++; structural = true; break;
            case WorldTarget::Keep: if (!t.rebuild_material) D.objects_kept++; break;
            case WorldTarget::Reinstance: D.objects_reinstanced++; any_reinstance = true; break;
            case WorldTarget::Resize: D.objects_reinstanced++; structural = true; break;
            }
            if (t.rebuild_material) { D.materials_rebuilt++; structural = true; }
            any_show |= t.show;
            if (t.live != (int)T.size()) structural = true;      // (the object is not where the target list wants it)
            T.push_back(t);
        }
    }
    for (char u : used) if (!u) { D.objects_removed++; structural = true; }
    const bool flags_change = c->sky_enabled != w.EnableSkydome || c->bg_enabled != w.EnableBackground;
    D.scene_changed = (structural || any_reinstance || any_show || plan.which || plan.clear || flags_change) ? 1u : 0u;

    // ---- commit.  The identities of the last frame go with the old world, as after a load; the identity table itself stands while the
    // objects and their order do.
    const bool ids_table_current = c->ids.table_gen == c->scene_gen;
    c->scene_gen++;
    if (!structural && ids_table_current) c->ids.table_gen = c->scene_gen;
    if (!D.scene_changed) {             // camera and lights at most: the uniforms, nothing else
        c->world = w;
        return world_uniforms(c, w, 0.0f, 0.0f, 0.0f);
    }
    // kept objects that stay the size they are: new values through the instance-update path, shown again through the visibility path
    for (const WorldTarget& t : T) {
        if (t.live < 0 || t.act == WorldTarget::Resize) continue;
        ZrSceneObject& o = c->objects[(size_t)t.live];
        if (t.act == WorldTarget::Reinstance) {
            o.host_stale = false;       // (every value is replaced: the host copy is the payload's from here on)
            rc = zr_object_set_instances(c, (uint32_t)t.live, 0, inst[t.desc].data(), o.n_inst);
            if (rc) return rc;
        }
        if (t.show) {
            if (o.hidden) { rc = zr_object_set_visible(c, (uint32_t)t.live, 1); if (rc) return rc; }
            if (o.instanced && (o.vis_stale || !o.vis.empty())) {
                const std::vector<uint8_t> ones(o.n_inst, 1);
                rc = zr_object_set_instance_visibility(c, (uint32_t)t.live, 0, ones.data(), o.n_inst);
                if (rc) return rc;
                o.vis.clear(); o.vis_stale = false;
            }
        }
    }
    if (structural) {
        // objects come, go, change size or place: behind everything in flight, and the next draw table carries the history over
        c->scene_dirty = true; c->history_remap = true; zr_casters_changed(c);
        if (zr_sync_all(c) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, "world update: device synchronisation failed");
        for (WorldTarget& t : T) {
            const ZrObjectDesc& d = w.ObjectDescs[t.desc];
            const ZrProfab& pf = c->profabs.find(d.ProfabName)->second[t.model];
            const std::vector<XkInstanceData>& in = inst[t.desc];
            if (t.act == WorldTarget::Add) {
                rc = zr_object_add_internal(c, pf.mesh, pf.mat, in.empty() ? nullptr : in.data(), (uint32_t)in.size());
                if (rc) return rc;
                t.live = (int)c->objects.size() - 1;
                world_tag(c->objects.back(), d.ProfabName, t.model);
                continue;
            }
            ZrSceneObject& o = c->objects[(size_t)t.live];
            if (t.act == WorldTarget::Resize) {
                rc = zr_object_remake_instances(c, o, in.empty() ? nullptr : in.data(), (uint32_t)in.size());
                if (rc) return rc;
                o.hidden = false;
            }
            if (t.rebuild_material) {
                rc = zr_object_remake_material(c, o, pf.mat);
                if (rc) return rc;
                o.mat_pristine = true;
            }
        }
        if (zr_sync_all(c) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, "world update: device synchronisation failed");
        std::vector<ZrSceneObject> next;      // the target order, by moving: no kept object's device memory is copied or freed
        next.reserve(T.size());
        for (const WorldTarget& t : T) next.push_back(std::move(c->objects[(size_t)t.live]));
        c->objects.swap(next);                // (what is left in `next` was removed: it releases its device memory here)
    }
    rc = zr_world_commit_overrides(c, plan);
    if (rc) return rc;
    c->world = w;
    zr_set_sky_flags(c, w.EnableSkydome ? 1 : 0, w.EnableBackground ? 1 : 0);
    rc = world_uniforms(c, w, 0.0f, 0.0f, 0.0f);
    if (rc) return rc;
    if (c->scene_dirty) {               // the draw table now, not at the next frame: the history is carried here (history_items)
        c->history_remap = true;
        rc = zr_scene_finalize(c);
        if (rc) return rc;
        D.history_items = (uint32_t)std::min<uint64_t>(c->history_items, 0xFFFFFFFFull);
    }
    return ZR_OK;
}

}  // namespace

// What instantiating a world throws becomes the world-load path's own codes ([WORLD] ..., ZR_ERR_STATE), inside the entry point's zr_guard.
int zr_apply_world_guarded(zr_ctx* c, const ZrWorld& w)
{
    try { return apply_world(c, w); }
    catch (const std::bad_alloc&) { return zr_fail(c, ZR_ERR_OOM, "[WORLD] out of host memory while building the scene"); }
    catch (const std::exception& e) { return zr_fail(c, ZR_ERR_STATE, std::string("[WORLD] ") + e.what()); }
}

// zr_world_update_json behind its parse, likewise: the refusal between the stages of a frame, the first update that is a load
int zr_update_world_guarded(zr_ctx* c, const ZrWorld& w, zr_world_delta& D)
{
    memset(&D, 0, sizeof D);
    D.struct_bytes = (uint32_t)sizeof D;
    if (int rc = zr_stage_idle(c, "zr_world_update_json")) return rc;
    if (hipSetDevice(c->device) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, "world update: no usable device");
    try {
        if (!c->world.loaded) {         // nothing to differ from: the update is a load
            D.differs = zr_world_diff(c->world, w); D.scene_changed = 1u;
            if (zr_sync_all(c) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, "world update: device synchronisation failed");
            const uint32_t before = (uint32_t)c->objects.size();
            const int rc = apply_world(c, w);
            if (rc == ZR_OK) { D.objects_removed = before; D.objects_added = (uint32_t)c->objects.size(); }
            return rc;
        }
        return update_world(c, w, D);
    }
    catch (const std::bad_alloc&) { return zr_fail(c, ZR_ERR_OOM, "[WORLD] out of host memory while updating the scene"); }
    catch (const std::exception& e) { return zr_fail(c, ZR_ERR_STATE, std::string("[WORLD] ") + e.what()); }
}

// ------------------------------------------------------------------------------------------------ C-ABI: world

extern "C" int zr_profab_register(zr_ctx* c, const char* name, uint32_t mesh_id, const zr_material* mat)
{
    if (!c || !name) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (mesh_id >= c->meshes.size()) return zr_fail(c, ZR_ERR_ARG, "bad mesh id");
        ZrProfab pf; pf.mesh = mesh_id;
        int rc = zr_material_prepare(c, mat, &pf.mat);
        if (rc) return rc;
        c->profabs[name].push_back(pf);
        return ZR_OK;
    });
}

extern "C" int zr_world_load_json(zr_ctx* c, const char* utf8, size_t len)
{
    if (!c || !utf8) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrWorld w; std::string err;
        if (!zr_world_parse(utf8, len, w, err)) return zr_fail(c, ZR_ERR_PARSE, err);
        (void)hipSetDevice(c->device);
        if (zr_sync_all(c) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, "world load: device synchronisation failed");
        return zr_apply_world_guarded(c, w);
    });
}

// The world applied as a difference: the matching rules and the contract are in include/zelda_render.h.
extern "C" int zr_world_update_json(zr_ctx* c, const char* utf8, size_t len, zr_world_delta* out, size_t bytes)
{
    if (!c || !utf8) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ZrWorld w; std::string err;
        if (!zr_world_parse(utf8, len, w, err)) return zr_fail(c, ZR_ERR_PARSE, err);
        zr_world_delta D;
        const int rc = zr_update_world_guarded(c, w, D);
        if (out) memcpy(out, &D, std::min(bytes, sizeof D));
        return rc;
    });
}

extern "C" int zr_world_json_diff(const char* a, size_t len_a, const char* b, size_t len_b, uint32_t* differs)
{
    if (!a || !b || !differs) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        ZrWorld wa, wb; std::string err;
        if (!zr_world_parse(a, len_a, wa, err) || !zr_world_parse(b, len_b, wb, err)) return ZR_ERR_PARSE;
        *differs = zr_world_diff(wa, wb);
        return ZR_OK;
    });
}

extern "C" int zr_world_save_json(zr_ctx* c, char* dst, size_t cap, size_t* len)
{
    if (!c || !len) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        const std::string o = zr_world_to_json(c->world);
        *len = o.size();
        if (dst) {
            if (cap < o.size()) return zr_fail(c, ZR_ERR_ARG, "buffer too small");
            memcpy(dst, o.data(), o.size());
        }
        return ZR_OK;
    });
}

// Context-free Load -> Save: parses a livelink payload / World.json with the same strictness as zr_world_load_json and
// writes it back in XkWorld::Save's layout.  Pure host code (no GPU): used to validate scenes before submission.
// On a parse/schema error returns ZR_ERR_PARSE and, if dst is given, the error text.
extern "C" int zr_world_json_normalize(const char* utf8, size_t len_in, char* dst, size_t cap, size_t* len)
{
    if (!utf8 || !len) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        ZrWorld w; std::string err;
        const bool ok = zr_world_parse(utf8, len_in, w, err);
        const std::string o = ok ? zr_world_to_json(w) : err;
        *len = o.size();
        if (dst) {
            if (cap < o.size()) return ZR_ERR_ARG;
            memcpy(dst, o.data(), o.size());
        }
        return ok ? ZR_OK : ZR_ERR_PARSE;
    });
}

// UpdateWorld + UpdateUniformBuffer (ZE:4294-4308, 4585-4664) from the loaded world's camera and lights: what the engine does every
// frame with its RollStage / RollLight / Time state.
extern "C" int zr_world_update_uniforms(zr_ctx* c, float roll_stage, float roll_light, float time)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->world.loaded) return zr_fail(c, ZR_ERR_STATE, "no world loaded");
        return world_uniforms(c, c->world, roll_stage, roll_light, time);
    });
}

extern "C" int zr_world_get_camera(zr_ctx* c, zr_camera* out)
{
    if (!c || !out) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        *out = c->world.MainCamera;
        return ZR_OK;
    });
}

extern "C" int zr_object_count(zr_ctx* c, uint32_t* n) { if (!c || !n) return ZR_ERR_ARG; return zr_guard(c, [&]() -> int { *n = (uint32_t)c->objects.size(); return ZR_OK; }); }

extern "C" int zr_object_get_instances(zr_ctx* c, uint32_t index, uint32_t* mesh_id, XkInstanceData* dst, uint32_t* n)
{
    if (!c || !n) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (index >= c->objects.size()) return zr_fail(c, ZR_ERR_ARG, "bad object index");
        const ZrSceneObject& o = c->objects[index];
        if (mesh_id) *mesh_id = o.mesh;
        *n = o.instanced ? o.n_inst : 0;
        if (dst && o.instanced && o.host_stale) { int rc = zr_instances_sync_host(c, c->objects[index]); if (rc) return rc; }
        if (dst && o.instanced) memcpy(dst, o.inst.data(), sizeof(XkInstanceData) * o.n_inst);
        return ZR_OK;
    });
}
