// zr_scene.cpp — scene upload behind the C-ABI (zelda_render.h): meshes and meshlets, materials and their mip chains, objects, the work
// pools and the draw table (zr_scene_finalize), skydome, background and cubemap.
//
// Host counterpart of XkZeldaEngineApp's CreateEngineScene (ZE:4140).
#include "zr_ctx.h"
#include "zr_math.h"
#include "zr_srgb.h"

#include <algorithm>
#include <cmath>
#include <cstring>

static const uint8_t kDefaultTexel[7][4] = {    // ZE:4951-4978: default_{grey,black,white,normal,white,black,white}.png
    {127,127,127,255}, {0,0,0,255}, {255,255,255,255}, {127,127,255,255}, {255,255,255,255}, {0,0,0,255}, {255,255,255,255}
};

float zr_srgb_decode8(uint32_t c)
{
    double x = (double)c / 255.0;
    double l = (x <= 0.04045) ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4);
    return (float)l;
}
// srgb_encode8: zr_srgb.h (the texture updates build their threshold table from the same function)

// ------------------------------------------------------------------------------------------------ scene

extern "C" int zr_mesh_create(zr_ctx* c, const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, uint32_t* mesh_id)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, v && idx && mesh_id && nv > 0 && ni > 0 && ni % 3 == 0);
        for (uint32_t i = 0; i < ni; ++i) if (idx[i] >= nv) return zr_fail(c, ZR_ERR_ARG, "index out of range");
        ZrMesh m;
        m.v.assign(v, v + nv); m.idx.assign(idx, idx + ni);
        c->meshes.push_back(std::move(m));
        *mesh_id = (uint32_t)c->meshes.size() - 1;
        return ZR_OK;
    });
}

static int validate_meshlets(zr_ctx* c, const ZrMesh& m, const XkMeshlet* ml, uint32_t nm, size_t nmv, const uint32_t* mv,
                             size_t nmt, const uint8_t* mt)
{
    for (uint32_t i = 0; i < nm; ++i) {
        if (ml[i].VertexCount == 0 || ml[i].VertexCount > 64 || ml[i].TriangleCount == 0 || ml[i].TriangleCount > 128)
            return zr_fail(c, ZR_ERR_ARG, "meshlet exceeds 64 vertices / 128 triangles");
        if ((size_t)ml[i].VertexOffset + ml[i].VertexCount > nmv || (size_t)ml[i].TriangleOffset + 3u * ml[i].TriangleCount > nmt)
            return zr_fail(c, ZR_ERR_ARG, "meshlet range out of bounds");
        for (uint32_t k = 0; k < ml[i].VertexCount; ++k)
            if (mv[ml[i].VertexOffset + k] >= m.v.size()) return zr_fail(c, ZR_ERR_ARG, "meshlet vertex index out of range");
        for (uint32_t k = 0; k < 3u * ml[i].TriangleCount; ++k)
            if (mt[ml[i].TriangleOffset + k] >= ml[i].VertexCount) return zr_fail(c, ZR_ERR_ARG, "meshlet triangle corner out of range");
    }
    return ZR_OK;
}

extern "C" int zr_mesh_set_meshlets(zr_ctx* c, uint32_t mesh_id, const XkMeshlet* ml, uint32_t nm, const uint32_t* mv, size_t nmv, const uint8_t* mt, size_t nmt)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size() && ml && nm && mv && mt);
        ZrMesh& m = c->meshes[mesh_id];
        if (m.uploaded) return zr_fail(c, ZR_ERR_STATE, "mesh already in use by a rendered scene");
        int rc = validate_meshlets(c, m, ml, nm, nmv, mv, nmt, mt);
        if (rc) return rc;
        // CreateMeshVertexBuffers<XkMeshIndirect> (ZE:4733-4756): the draw becomes "meshlet by meshlet"; rebuild the
        // draw-order index buffer accordingly so primitive ids follow meshlet order.
        m.ms.meshlets.assign(ml, ml + nm); m.ms.mverts.assign(mv, mv + nmv); m.ms.mtris.assign(mt, mt + nmt);
        // Every cull trusts the bounding sphere to enclose the meshlet's vertices (and the cone to describe its triangles): a record
        // whose sphere does not is recomputed (ZM:149-166 fills them from meshopt_computeMeshletBounds, so a sound file never is).
        for (uint32_t i = 0; i < nm; ++i) {
            XkMeshlet& d = m.ms.meshlets[i];
            bool ok = std::isfinite(d.BoundsRadius) && d.BoundsRadius >= 0.0f;
            for (uint32_t k = 0; ok && k < d.VertexCount; ++k) {
                const float* q = m.v[mv[d.VertexOffset + k]].Position;
                const double dx = (double)q[0] - d.BoundsCenter[0], dy = (double)q[1] - d.BoundsCenter[1], dz = (double)q[2] - d.BoundsCenter[2];
                if (!(std::sqrt(dx * dx + dy * dy + dz * dz) <= (double)d.BoundsRadius * (1.0 + 1e-5) + 1e-30)) ok = false;
            }
            if (!ok) {
                XkMeshlet b = d;
                zr_meshlet_bounds(m.v.data(), mv + d.VertexOffset, d.VertexCount, mt + d.TriangleOffset, d.TriangleCount, &b);
                d = b;
            }
        }
        m.ms.tri_order.clear(); m.idx.clear();
        uint32_t base = 0;
        for (uint32_t i = 0; i < nm; ++i) {
            XkMeshlet& d = m.ms.meshlets[i];
            d.BindlessContext = base;
            for (uint32_t t = 0; t < d.TriangleCount; ++t) {
                for (int k = 0; k < 3; ++k) m.idx.push_back(mv[d.VertexOffset + mt[d.TriangleOffset + 3u * t + (uint32_t)k]]);
                m.ms.tri_order.push_back(base + t);
            }
            base += d.TriangleCount;
        }
        m.has_meshlets = true; zr_casters_changed(c);
        return ZR_OK;
    });
}

extern "C" int zr_mesh_build_meshlets(zr_ctx* c, uint32_t mesh_id, uint32_t max_v, uint32_t max_t, float cone_weight)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size());
        if (max_v == 0) max_v = 64;
        if (max_t == 0) max_t = 124;
        ARGCHK(c, max_v >= 3 && max_v <= 64 && max_t >= 1 && max_t <= 128);
        ZrMesh& m = c->meshes[mesh_id];
        if (m.uploaded) return zr_fail(c, ZR_ERR_STATE, "mesh already in use by a rendered scene");
        zr_build_meshlets(m.v.data(), (uint32_t)m.v.size(), m.idx.data(), (uint32_t)m.idx.size(), max_v, max_t, cone_weight, &m.ms);
        m.has_meshlets = true; zr_casters_changed(c);
        return ZR_OK;
    });
}

// Context-free form of the clusteriser: the ZeldaMeshlet tool's BuildMeshlets (ZM:132-172) as a library call.  Pure host
// code (runs without a GPU).  Pass NULL outputs to query the sizes.  tri_order[k] = index-buffer triangle of slot k.
extern "C" int zr_meshlets_build(const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, uint32_t max_v, uint32_t max_t, float cone_weight, XkMeshlet* ml, uint32_t* nm, uint32_t* mv, size_t* nmv, uint8_t* mt, size_t* nmt, uint32_t* tri_order)
{
    if (!v || !idx || !nm || !nmv || !nmt || nv == 0 || ni == 0 || ni % 3) return ZR_ERR_ARG;
    return zr_guard(nullptr, [&]() -> int {
        if (max_v == 0) max_v = 64;
        if (max_t == 0) max_t = 124;
        if (max_v < 3 || max_v > 64 || max_t < 1 || max_t > 128) return ZR_ERR_ARG;
        for (uint32_t i = 0; i < ni; ++i) if (idx[i] >= nv) return ZR_ERR_ARG;
        ZrMeshletSet ms;
        zr_build_meshlets(v, nv, idx, ni, max_v, max_t, cone_weight, &ms);
        *nm = (uint32_t)ms.meshlets.size(); *nmv = ms.mverts.size(); *nmt = ms.mtris.size();
        if (ml) { memcpy(ml, ms.meshlets.data(), ms.meshlets.size() * sizeof(XkMeshlet)); for (uint32_t i = 0; i < *nm; ++i) ml[i].BindlessContext = 0; }
        if (mv) memcpy(mv, ms.mverts.data(), ms.mverts.size() * 4);
        if (mt) memcpy(mt, ms.mtris.data(), ms.mtris.size());
        if (tri_order) memcpy(tri_order, ms.tri_order.data(), ms.tri_order.size() * 4);
        return ZR_OK;
    });
}

extern "C" int zr_mesh_get_meshlets(zr_ctx* c, uint32_t mesh_id, XkMeshlet* ml, uint32_t* nm, uint32_t* mv, size_t* nmv, uint8_t* mt, size_t* nmt)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size());
        ZrMesh& m = c->meshes[mesh_id];
        if (ml) { int rc = zr_mesh_sync_host(c, m, true); if (rc) return rc; }      // (after vertex updates: the bounds of the current vertices)
        if (nm) *nm = (uint32_t)m.ms.meshlets.size();
        if (nmv) *nmv = m.ms.mverts.size();
        if (nmt) *nmt = m.ms.mtris.size();
        if (ml) { memcpy(ml, m.ms.meshlets.data(), m.ms.meshlets.size() * sizeof(XkMeshlet));
                  for (size_t i = 0; i < m.ms.meshlets.size(); ++i) ml[i].BindlessContext = 0; }
        if (mv) memcpy(mv, m.ms.mverts.data(), m.ms.mverts.size() * 4);
        if (mt) memcpy(mt, m.ms.mtris.data(), m.ms.mtris.size());
        return ZR_OK;
    });
}

int zr_material_prepare(zr_ctx* c, const zr_material* mat, ZrMaterialHost* out)
{
    for (int t = 0; t < 7; ++t) {
        const uint8_t* px = kDefaultTexel[t];
        out->image[t].clear(); out->w[t] = out->h[t] = 1;
        if (mat && mat->tex[t].rgba8) {
            const zr_image& im = mat->tex[t];
            if (im.width == 0 || im.height == 0 || im.width > 16384 || im.height > 16384) return zr_fail(c, ZR_ERR_ARG, "bad material image size");
            const size_t n = (size_t)im.width * im.height * 4;
            bool constant = true;
            for (size_t i = 4; i < n; ++i) if (im.rgba8[i] != im.rgba8[i & 3]) { constant = false; break; }
            px = im.rgba8;
            if (!constant) { out->image[t].assign(im.rgba8, im.rgba8 + n); out->w[t] = im.width; out->h[t] = im.height; }
        }
        out->texel[t] = (uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16 | (uint32_t)px[3] << 24;
    }
    for (int k = 0; k < 3; ++k) out->bc_linear[k] = zr_srgb_decode8((out->texel[0] >> (8 * k)) & 255u);
    return ZR_OK;
}

static int idx_clamp_h(float f, int hi) { f = fminf(fmaxf(f, 0.0f), (float)hi); return (int)f; }

// RHIGenerateMipmaps (ZE:6348-6433): level l+1 = vkCmdBlitImage(LINEAR) of level l at half size; mipLevels =
// floor(log2(max(w, h))) + 1 (ZE:6887).  Filtered on decoded values (sRGB for the base-colour slot, ZE:5878), re-encoded.
static void build_mip_chain(const zr_ctx* c, const uint8_t* rgba8, uint32_t w, uint32_t h, bool srgb, std::vector<uint8_t>* chain, uint32_t* levels)
{
    uint32_t m = w > h ? w : h;
    uint32_t nl = 1; while (m > 1) { m >>= 1; nl++; }
    *levels = nl;
    chain->assign(rgba8, rgba8 + (size_t)w * h * 4);
    size_t src_off = 0;
    uint32_t sw = w, sh = h;
    for (uint32_t l = 1; l < nl; ++l) {
        const uint32_t dw = zr_mip_next(sw), dh = zr_mip_next(sh);
        const size_t dst_off = chain->size();
        chain->resize(dst_off + (size_t)dw * dh * 4);
        const uint8_t* src = chain->data() + src_off;
        uint8_t* dst = chain->data() + dst_off;
        const float kx = (float)sw / (float)dw, ky = (float)sh / (float)dh;
        for (uint32_t y = 0; y < dh; ++y) for (uint32_t x = 0; x < dw; ++x) {
            const float fu = fmaf((float)x + 0.5f, kx, -0.5f), fv = fmaf((float)y + 0.5f, ky, -0.5f);
            const float fx = floorf(fu), fy = floorf(fv), a = fu - fx, b = fv - fy;
            const int x0 = idx_clamp_h(fx, (int)sw - 1), x1 = idx_clamp_h(fx + 1.0f, (int)sw - 1);
            const int y0 = idx_clamp_h(fy, (int)sh - 1), y1 = idx_clamp_h(fy + 1.0f, (int)sh - 1);
            const uint8_t* p00 = src + ((size_t)y0 * sw + x0) * 4; const uint8_t* p10 = src + ((size_t)y0 * sw + x1) * 4;
            const uint8_t* p01 = src + ((size_t)y1 * sw + x0) * 4; const uint8_t* p11 = src + ((size_t)y1 * sw + x1) * 4;
            for (int ch = 0; ch < 4; ++ch) {
                const bool sr = srgb && ch < 3;
                const float t00 = sr ? c->lut[p00[ch]] : (float)p00[ch] / 255.0f, t10 = sr ? c->lut[p10[ch]] : (float)p10[ch] / 255.0f;
                const float t01 = sr ? c->lut[p01[ch]] : (float)p01[ch] / 255.0f, t11 = sr ? c->lut[p11[ch]] : (float)p11[ch] / 255.0f;
                const float top = fmaf(a, t10 - t00, t00), bot = fmaf(a, t11 - t01, t01);
                const float v = fmaf(b, bot - top, top);
                dst[((size_t)y * dw + x) * 4 + ch] = sr ? srgb_encode8(v) : (uint8_t)zr_unorm(v, 255.0f);
            }
        }
        src_off = dst_off; sw = dw; sh = dh;
    }
}

// An image for the kernels to sample: `bytes` into device memory of `own` (ZrOwn::alloc_image)
static int upload_bytes(zr_ctx* c, ZrOwn& own, const std::vector<uint8_t>& bytes, uint8_t** d)
{
    HIPCHK(c, own.alloc_image(d, bytes.size()));
    HIPCHK(c, hipMemcpy(*d, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    return ZR_OK;
}
// ... an RGBA8 image with its mip chain; `chain` (optional) keeps the chain on the host, for the packed material
static int upload_image(zr_ctx* c, ZrOwn& own, const uint8_t* rgba8, uint32_t iw, uint32_t ih, bool srgb, uint8_t** d, uint32_t* w, uint32_t* h,
                        uint32_t* levels, std::vector<uint8_t>* chain = nullptr)
{
    if (iw == 0 || ih == 0 || iw > 16384 || ih > 16384) return zr_fail(c, ZR_ERR_ARG, "bad image size");
    std::vector<uint8_t> mine;
    if (!chain) chain = &mine;
    build_mip_chain(c, rgba8, iw, ih, srgb, chain, levels);
    *w = iw; *h = ih;
    return upload_bytes(c, own, *chain, d);
}

// The material's images of `o`: mip chains and the packed form, into o.tex_mem (released first: a world update rebuilds a material here)
int zr_object_remake_material(zr_ctx* c, ZrSceneObject& o, const ZrMaterialHost& mat)
{
    o.tex_mem.release();
    for (int t = 0; t < 8; ++t) { o.d_tex[t] = nullptr; o.tex_w[t] = o.tex_h[t] = o.tex_levels[t] = 0; }
    o.mixed_sizes = false;
    memcpy(o.texel, mat.texel, sizeof o.texel); memcpy(o.bc_linear, mat.bc_linear, sizeof o.bc_linear);
    std::vector<uint8_t> chains[7];
    int lead = -1;                                          // first slot that holds an image
    for (int t = 0; t < 7; ++t) {
        if (mat.image[t].empty()) continue;
        int rc = upload_image(c, o.tex_mem, mat.image[t].data(), mat.w[t], mat.h[t], t == 0, &o.d_tex[t], &o.tex_w[t], &o.tex_h[t], &o.tex_levels[t], &chains[t]);
        if (rc) return rc;
        if (lead < 0) lead = t;
        else if (mat.w[t] != mat.w[lead] || mat.h[t] != mat.h[lead]) o.mixed_sizes = true;
    }
    if (lead >= 0 && !o.mixed_sizes) {
        // The packed material: per texel of the (common) mip chain the 13 channels BaseScene.frag reads, 16 B (ZR_PK_*); constant slots
        // put their constant there (the resolve takes those from the draw record, not from here).
        const size_t n_texels = chains[lead].size() / 4;
        std::vector<uint8_t> pk(n_texels * 16, 0);
        for (int slot = 0; slot < 7; ++slot) {
            const auto& k = kSlotPack[slot];
            const bool image = !chains[slot].empty();
            const uint8_t* src = image ? chains[slot].data() : nullptr;
            for (size_t i = 0; i < n_texels; ++i)
                for (uint32_t ch = 0; ch < k.n; ++ch)
                    pk[i * 16 + k.ch + ch] = image ? src[i * 4 + ch] : (uint8_t)(mat.texel[slot] >> (8 * ch));
        }
        int rc = upload_bytes(c, o.tex_mem, pk, &o.d_tex[7]);
        if (rc) return rc;
        o.tex_w[7] = mat.w[lead]; o.tex_h[7] = mat.h[lead]; o.tex_levels[7] = o.tex_levels[lead];
    }
    return ZR_OK;
}

// The instance buffers of `o` from n_inst values (0: one identity record, not instanced), into o.mem (released first, and with it the
// update and visibility state: a world update re-makes an object of another instance count here).  Enqueued on the host's stream.
int zr_object_remake_instances(zr_ctx* c, ZrSceneObject& o, const XkInstanceData* inst, uint32_t n_inst)
{
    o.mem.release();
    o.d_inst = nullptr; o.d_raw = nullptr; o.upd = {}; o.pending[0] = o.pending[1] = 0; o.tab1 = false; o.host_stale = false;
    o.flag_pending[0] = o.flag_pending[1] = false; o.vis_stale = false; o.vis.clear();
    o.instanced = n_inst > 0; o.n_inst = n_inst ? n_inst : 1;
    o.inst.clear();
    if (n_inst) o.inst.assign(inst, inst + n_inst);
    HIPCHK(c, o.mem.alloc(&o.d_inst, o.n_inst));
    if (n_inst) {                       // (kept: the authoritative values of zr_object_set_instances / zr_object_update_instances_async)
        HIPCHK(c, o.mem.alloc(&o.d_raw, n_inst));
        HIPCHK(c, hipMemcpyAsync(o.d_raw, inst, sizeof(XkInstanceData) * n_inst, hipMemcpyHostToDevice, c->stream));
    }
    zr_launch_instance_prep(o.d_raw, o.d_inst, o.n_inst, o.instanced ? 1u : 0u, c->stream);
    return ZR_OK;
}

int zr_object_add_internal(zr_ctx* c, uint32_t mesh_id, const ZrMaterialHost& mat, const XkInstanceData* inst, uint32_t n_inst)
{
    ZrSceneObject o;
    o.mesh = mesh_id;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = zr_object_remake_material(c, o, mat);         // (a failure below drops `o`, and with it what it has made)
    if (rc == ZR_OK) rc = zr_object_remake_instances(c, o, inst, n_inst);
    if (rc) return rc;
    HIPCHK(c, zr_sync_all(c));
    c->objects.push_back(std::move(o));
    c->scene_dirty = true; c->scene_gen++; zr_casters_changed(c);
    return ZR_OK;
}

extern "C" int zr_object_add(zr_ctx* c, uint32_t mesh_id, const zr_material* mat, const XkInstanceData* inst, uint32_t n_inst)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        ARGCHK(c, mesh_id < c->meshes.size() && (n_inst == 0 || inst));
        ZrMaterialHost m;
        int rc = zr_material_prepare(c, mat, &m);
        if (rc) return rc;
        return zr_object_add_internal(c, mesh_id, m, inst, n_inst);
    });
}

// Capacities of the triangle-record arrays (chunks of 256 records) and of the clipped-triangle list, for hosts that size them themselves
// (0 = the default: 16 records per meshlet-instance, at least 32 Mi; 2^18 triangles).  Takes effect at the next frame.  The arrays hold at
// most 2^30 - 1 records (the kernels index them with 32-bit words): record_chunks beyond ZR_MAX_RECORD_CHUNKS is refused.
static constexpr uint32_t ZR_MAX_RECORD_CHUNKS = 0x3FFFFFFFu / 256u;
extern "C" int zr_set_limits(zr_ctx* c, uint32_t record_chunks, uint32_t slow_triangles)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (record_chunks > ZR_MAX_RECORD_CHUNKS) return zr_fail(c, ZR_ERR_ARG, "zr_set_limits: record_chunks above (2^30 - 1) / 256");
        c->limit_record_chunks = record_chunks; c->limit_slow_triangles = slow_triangles;
        c->work_capacity = 0; c->scene_dirty = true;          // the pools are re-made by the next frame
        zr_casters_changed(c);                                // (the shadow bins and the slow list with them)
        return ZR_OK;
    });
}

extern "C" int zr_set_bucket_share(zr_ctx* c, uint32_t percent)
{
    if (!c || percent < 1u || percent > 100u) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->bucket_pct = percent;          // (k_plan's argument from the next plan on; a frame that overflows its buckets is the same frame.
                                          // The camera pass's record buckets only: the shadow bins know nothing of it, the map is kept)
        zr_camera_changed(c);             // (where the records go: round 2 is drawn again, pool_used is the new layout's)
        return ZR_OK;
    });
}


// (every object and mesh releases its device memory as it goes)
static void free_scene(zr_ctx* c)
{
    c->objects.clear(); c->scene_gen++; zr_casters_changed(c);
    c->meshes.clear();
    c->profabs.clear();
    zr_drop_draw_tables(c);
    c->n_objs = 0; c->n_work = 0; c->scene_dirty = true;
}

extern "C" int zr_scene_clear(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        free_scene(c);
        return ZR_OK;
    });
}

static int upload_mesh(zr_ctx* c, ZrMesh& m)
{
    if (m.uploaded) return ZR_OK;
    m.mem.release();                    // (what an upload that failed part-way made)
    if (!m.has_meshlets) {
        zr_build_meshlets(m.v.data(), (uint32_t)m.v.size(), m.idx.data(), (uint32_t)m.idx.size(), 64, 124, 0.2f, &m.ms);
        m.has_meshlets = true;
    }
    // whole-mesh bounding sphere (centroid + max distance)
    double cx = 0, cy = 0, cz = 0;
    for (auto& v : m.v) { cx += v.Position[0]; cy += v.Position[1]; cz += v.Position[2]; }
    cx /= (double)m.v.size(); cy /= (double)m.v.size(); cz /= (double)m.v.size();
    double r = 0;
    for (auto& v : m.v) { double dx = v.Position[0] - cx, dy = v.Position[1] - cy, dz = v.Position[2] - cz; r = std::max(r, std::sqrt(dx * dx + dy * dy + dz * dz)); }
    m.center[0] = (float)cx; m.center[1] = (float)cy; m.center[2] = (float)cz; m.radius = (float)(r * 1.0001) + 1e-30f;
    // flatten for the kernels: one coalesced 16 B load per meshlet vertex, one 8 B load per meshlet triangle
    std::vector<float4> mpos(m.ms.mverts.size());
    for (size_t i = 0; i < mpos.size(); ++i) {
        const float* p = m.v[m.ms.mverts[i]].Position;
        mpos[i] = make_float4(p[0], p[1], p[2], 1.0f);
    }
    std::vector<uint2> mtri(m.ms.tri_order.size());
    for (const XkMeshlet& ml : m.ms.meshlets)
        for (uint32_t t = 0; t < ml.TriangleCount; ++t) {
            const uint8_t* tp = m.ms.mtris.data() + ml.TriangleOffset + 3u * t;
            mtri[ml.BindlessContext + t] = make_uint2((uint32_t)tp[0] | (uint32_t)tp[1] << 8 | (uint32_t)tp[2] << 16,
                                                      m.ms.tri_order[ml.BindlessContext + t]);
        }
    std::vector<ZrRVertex> rv(m.v.size());             // the resolve's vertex record: position + uv + the normalised normal
    for (size_t i = 0; i < rv.size(); ++i) {
        const XkVertex& x = m.v[i];
        const zf3 n = zr_normalize(zr3(x.Normal[0], x.Normal[1], x.Normal[2]));
        rv[i] = ZrRVertex{ x.Position[0], x.Position[1], x.Position[2], x.TexCoord[0], n.x, n.y, n.z, x.TexCoord[1] };
    }
    // ... and the same records per TRIANGLE CORNER in draw order (96 bytes a triangle): the resolve reaches a pixel's three corners from the
    // primitive id in one round trip instead of two (index, then vertex) - the kernel waits for its chain of dependent loads, not for arithmetic
    std::vector<ZrRVertex> rt(std::max<size_t>(1, m.idx.size()));
    for (size_t i = 0; i < m.idx.size(); ++i) rt[i] = rv[m.idx[i]];
    HIPCHK(c, upload(m.mem, &m.d_rt, rt));
    HIPCHK(c, upload(m.mem, &m.d_v, m.v)); HIPCHK(c, upload(m.mem, &m.d_rv, rv)); HIPCHK(c, upload(m.mem, &m.d_idx, m.idx)); HIPCHK(c, upload(m.mem, &m.d_meshlets, m.ms.meshlets));
    // draw-order triangle -> meshlet (the resolve marks the meshlet-instances that own a pixel)
    std::vector<uint32_t> tri_meshlet(std::max<size_t>(1, m.idx.size() / 3), 0u);
    for (size_t mi = 0; mi < m.ms.meshlets.size(); ++mi) {
        const XkMeshlet& ml = m.ms.meshlets[mi];
        for (uint32_t t = 0; t < ml.TriangleCount; ++t) {
            const uint32_t tri = m.ms.tri_order[ml.BindlessContext + t];
            if (tri < tri_meshlet.size()) tri_meshlet[tri] = (uint32_t)mi;
        }
    }
    std::vector<float4> mbox(2 * std::max<size_t>(1, m.ms.meshlets.size()), make_float4(0.0f, 0.0f, 0.0f, 0.0f));   // object-space box per meshlet
    for (size_t mi = 0; mi < m.ms.meshlets.size(); ++mi) {
        const XkMeshlet& ml = m.ms.meshlets[mi];
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (uint32_t v = 0; v < ml.VertexCount; ++v) {
            const float4& q = mpos[ml.VertexOffset + v];
            const float e[3] = { q.x, q.y, q.z };
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], e[a]); hi[a] = std::max(hi[a], e[a]); }      // (a NaN coordinate drops out: k_geom sees it)
        }
        mbox[2 * mi] = make_float4(lo[0], lo[1], lo[2], 0.0f); mbox[2 * mi + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
    HIPCHK(c, upload(m.mem, &m.d_mpos, mpos)); HIPCHK(c, upload(m.mem, &m.d_mbox, mbox)); HIPCHK(c, upload(m.mem, &m.d_mtri, mtri)); HIPCHK(c, upload(m.mem, &m.d_tri_meshlet, tri_meshlet));
    m.uploaded = true;
    return ZR_OK;
}

// The work pools' per-tile parts (zr_ctx.h): the shadow pass's work-unit table, the camera pass's per-tile bucket tables, cursors, round-2
// counts and work-unit table - made through `into`, zeroed, and handed back in *T / *chunk_tab / *chunk_capacity.  The context itself is
// not touched: make_work_pools and zr_resize put the result in place.
int zr_make_pool_tiles(zr_ctx* c, ZrOwn& into, uint32_t n_tiles, ZrTriBins* T, uint4** chunk_tab, uint32_t* chunk_capacity)
{
    *chunk_capacity = c->bin_capacity / ZR_CHUNK + std::max(n_tiles, c->sn_tiles) + 1u;
    HIPCHK(c, into.alloc(chunk_tab, *chunk_capacity));
    T->n_tiles = n_tiles;
    T->unit_cap = T->bucket_max / (ZR_TCHUNK * ZR_TBATCHES) + 2u * n_tiles + 1u;
    HIPCHK(c, into.alloc(&T->tile_base, n_tiles)); HIPCHK(c, into.alloc(&T->tile_cap, n_tiles));
    HIPCHK(c, into.alloc(&T->cursor, (size_t)2 * n_tiles * ZR_TSTRIDE));
    HIPCHK(c, into.alloc(&T->unit_tab, T->unit_cap)); HIPCHK(c, into.alloc(&T->r2_count, n_tiles));
    // (no plan yet: every bucket is empty - the first frame counts before it draws, see gbuffer_pass.  A fill that landed after the next
    // frame's k_plan would wipe the plan - every record then overflows into sections of capacity 0)
    HIPCHK(c, zr_fill_sync({ { T->tile_base, 0, (size_t)n_tiles * 4 }, { T->tile_cap, 0, (size_t)n_tiles * 4 },
                             { T->cursor, 0, (size_t)2 * n_tiles * ZR_TSTRIDE * 4 }, { T->r2_count, 0, (size_t)n_tiles * 4 } }));
    return ZR_OK;
}
// ... and the few words of plan state that are no tile's: as a scene's first frame finds them
hipError_t zr_pool_plan_reset(zr_ctx* c)
{
    const ZrTriBins& T = c->tb;
    return zr_fill_sync({ { T.over_cursor, 0, 2 * ZR_OVER_SECTIONS * 4 }, { T.n_units, 0, 4 }, { T.plan, 0, 8 }, { T.r2_stats, 0, ZR_R2_WORDS * 4 } });
}

// The work pools for cap_w meshlet-instances: the cull's lists, the shadow pass's bins, the camera pass's triangle records, the occlusion
// tests' boxes and flags.  A failed allocation returns with work_capacity 0 (and the caller's scene_dirty still set): the next frame
// tries again instead of launching on freed buffers.
static int make_work_pools(zr_ctx* c, uint32_t cap_w)
{
    ZrOwn& P = c->pools;
    P.release(); c->pool_tiles.release();
    c->work_capacity = 0; zr_history_forgotten(c, ZR_HIST_PLAN);
    for (auto& o : c->objects) o.work_valid = false;      // (the history lived in the pools: zr_scene_finalize reads it before it comes here)
    for (auto& sc : c->sc) sc = {};
    c->sb.bins = nullptr; c->sb.chunk_tab = nullptr; c->tb = {};
    c->d_pxrect = nullptr; c->d_zmin = nullptr; c->d_visflag[0] = c->d_visflag[1] = nullptr; c->d_spxrect = nullptr; c->d_szmin = nullptr; c->d_sflag = nullptr;
    const uint64_t cap = std::max<uint64_t>(1u << 20, 8ull * cap_w);
    c->bin_capacity = (uint32_t)std::min<uint64_t>(cap, 0x3FFFFFFFull);
    for (auto& sc : c->sc) { HIPCHK(c, P.alloc(&sc.rects, cap_w)); HIPCHK(c, P.alloc(&sc.work, cap_w)); }
    HIPCHK(c, P.alloc(&c->sb.bins, c->bin_capacity));
    // triangle-binned camera pass: triangle records (32 B) live in per-tile BUCKETS of two 16-byte planes, laid out every frame by
    // k_plan from the previous frame's per-tile counts; what lies behind the last bucket is the frame's overflow region (what a tile gets
    // beyond its bucket).  Sized from the scene: 16 records per meshlet-instance, at least 32 Mi - 1 GB of 288 reserved, touched as far as a frame
    // needs.  Planes that run full are reported like a bin overflow (zr_set_limits sizes them: 256 records per "chunk", at most 2^30 - 1 records).
    ZrTriBins& T = c->tb;
    T.n_waves = 8192; T.slow_cap = 1u << 18;
    // (16 per meshlet-instance: the frame after a camera cut at config 4 puts ~ 60 M records - 5 per meshlet-instance - into the 64
    // sections of the overflow region, unevenly; with 8 the fullest section ran over.  6 GB of 288 at 1 M instances.)
    uint64_t n_rec = std::min<uint64_t>(std::max<uint64_t>(32ull << 20, 16ull * cap_w), 0x3FFFFFFFull);
    if (c->limit_record_chunks) n_rec = 256ull * c->limit_record_chunks;      // zr_set_limits (a host sizing the planes; the overflow tests)
    if (c->limit_slow_triangles) T.slow_cap = std::max(2u, c->limit_slow_triangles);
    T.n_rec = (uint32_t)n_rec; T.bucket_max = (uint32_t)(n_rec - n_rec / 8u);
    if (int rc = zr_make_pool_tiles(c, c->pool_tiles, c->n_tiles, &T, &c->sb.chunk_tab, &c->chunk_capacity)) return rc;
    HIPCHK(c, P.alloc(&T.sel, cap_w)); HIPCHK(c, P.alloc(&T.recA, (size_t)n_rec)); HIPCHK(c, P.alloc(&T.recB, (size_t)n_rec));
    HIPCHK(c, P.alloc(&T.over_tile, (size_t)n_rec)); HIPCHK(c, P.alloc(&T.plan, 2));
    HIPCHK(c, P.alloc(&T.over_cursor, 2 * ZR_OVER_SECTIONS)); HIPCHK(c, P.alloc(&T.n_units, 1));
    HIPCHK(c, P.alloc(&T.wave_culled, T.n_waves)); HIPCHK(c, P.alloc(&T.slow, 4ull * T.slow_cap));
    HIPCHK(c, P.alloc(&T.r2_stats, ZR_R2_WORDS));
    HIPCHK(c, P.alloc(&c->d_pxrect, cap_w)); HIPCHK(c, P.alloc(&c->d_zmin, cap_w));
    HIPCHK(c, P.alloc(&c->d_visflag[0], cap_w)); HIPCHK(c, P.alloc(&c->d_visflag[1], cap_w));
    HIPCHK(c, P.alloc(&c->d_spxrect, cap_w)); HIPCHK(c, P.alloc(&c->d_szmin, cap_w)); HIPCHK(c, P.alloc(&c->d_sflag, cap_w));
    HIPCHK(c, zr_pool_plan_reset(c));
    HIPCHK(c, zr_fill_sync({ { c->d_visflag[0], 0, cap_w }, { c->d_visflag[1], 0, cap_w } }));      // (no frame's stamp is 0)
    c->work_capacity = cap_w;              // every buffer is there
    return ZR_OK;
}

// CreateEngineScene's GPU half (ZE:4140-4284): meshlets, buffers, draw table in the reference's draw order
int zr_scene_finalize(zr_ctx* c)
{
    if (!c->scene_dirty) return ZR_OK;
    HIPCHK(c, zr_sync_all(c));
    for (auto& o : c->objects) { int rc = upload_mesh(c, c->meshes[o.mesh]); if (rc) return rc; }
    const bool sky = c->sky_set && c->sky_enabled;
    if (sky) { int rc = upload_mesh(c, c->sky_mesh); if (rc) return rc; }
    std::vector<ZrObject> tab;
    uint64_t work = 0, prim = 0, inst_total = 0;
    const uint32_t old_work = c->n_work;      // (the numbering the history on the device was written in)
    auto emit = [&](ZrSceneObject& o, const ZrMesh& m, uint32_t flags) {
        ZrObject d; memset(&d, 0, sizeof d);
        o.draw = (uint32_t)tab.size();
        d.verts = m.d_v; d.rverts = m.d_rv; d.rtris = m.d_rt; d.indices = m.d_idx; d.meshlets = m.d_meshlets; d.mpos = m.d_mpos; d.mbox = m.d_mbox; d.mtri = m.d_mtri; d.tri_meshlet = m.d_tri_meshlet;
        d.inst = o.d_inst;
        d.n_meshlets = (uint32_t)m.ms.meshlets.size(); d.n_tris = (uint32_t)(m.idx.size() / 3);
        d.n_inst = o.n_inst; d.instanced = o.instanced; d.flags = flags;
        d.work_base = (uint32_t)work; d.prim_base = (uint32_t)prim; d.inst_base = (uint32_t)inst_total;
        inst_total += d.n_inst;
        memcpy(d.texel, o.texel, sizeof d.texel); memcpy(d.bc_linear, o.bc_linear, sizeof d.bc_linear);
        for (int t = 0; t < 7; ++t)
            for (int ch = 0; ch < 4; ++ch) {
                const uint32_t v8 = (o.texel[t] >> (8 * ch)) & 255u;
                d.texc[t][ch] = (t == 0 && ch < 3) ? c->lut[v8] : (float)v8 / 255.0f;
            }
        for (int t = 0; t < 7; ++t) { d.tex[t].data = o.d_tex[t]; d.tex[t].w = o.tex_w[t]; d.tex[t].h = o.tex_h[t]; d.tex[t].levels = o.tex_levels[t]; d.tex[t]._pad = 0; }
        d.packed.data = o.d_tex[7]; d.packed.w = o.tex_w[7]; d.packed.h = o.tex_h[7]; d.packed.levels = o.tex_levels[7]; d.packed._pad = 0;
        memcpy(d.mesh_center, m.center, sizeof d.mesh_center); d.mesh_radius = m.radius;
        // BaseScene.frag on constant slots, once per draw instead of once per pixel (the kernels' own arithmetic: zr_math.h)
        for (int t = 0; t < 7; ++t) if (!o.d_tex[t]) d.const_slots |= 1u << t;
        const zf3 ts = zr_tangent_space_normal(zr3(d.texc[3][0], d.texc[3][1], d.texc[3][2]));
        d.ts_const[0] = ts.x; d.ts_const[1] = ts.y; d.ts_const[2] = ts.z;
        d.c_scene_color = zr_unorm(d.texc[5][0], 255.0f) | zr_unorm(d.texc[5][1], 255.0f) << 8 | zr_unorm(d.texc[5][2], 255.0f) << 16 | zr_unorm(d.texc[6][0], 255.0f) << 24;
        d.c_gB = zr_unorm(d.texc[1][0], 255.0f) | zr_unorm(1.0f, 255.0f) << 8 | zr_unorm(fmaxf(0.01f, d.texc[2][0]), 255.0f) << 16 | 255u << 24;
        d.c_gC = zr_unorm(d.texc[0][0], 255.0f) | zr_unorm(d.texc[0][1], 255.0f) << 8 | zr_unorm(d.texc[0][2], 255.0f) << 16 | zr_unorm(d.texc[4][0], 255.0f) << 24;
        work += (uint64_t)d.n_meshlets * d.n_inst; prim += (uint64_t)d.n_tris * d.n_inst;
        tab.push_back(d);
    };
    for (int pass = 0; pass < 2; ++pass)                 // non-instanced draws, then instanced draws (ZE:3445-3476)
        for (auto& o : c->objects)
            if ((int)o.instanced == pass) emit(o, c->meshes[o.mesh], o.hidden ? ZR_OBJ_HIDDEN : 0u);
    // The skydome is the table's last record but no work item of the shadow or the deferred-scene pass: it is drawn after the lighting
    // quad (ZE:3681-3691), depth-tested against the scene and colour only - k_sky_tiles + the resolve.
    const uint64_t scene_work = work, scene_inst = inst_total;
    if (sky) emit(c->sky_obj, c->sky_mesh, ZR_OBJ_SKY);
    if (work >= 0xFFFFFFFFull || prim >= 0xFFFFFFFFull) return zr_fail(c, ZR_ERR_OVERFLOW, "scene exceeds 2^32 meshlet-instances or primitives");
    zr_drop_draw_tables(c);             // (zr_update_table: table 1)
    HIPCHK(c, upload(c->tables, &c->d_objs_b[0], tab));
    c->d_objs = c->d_objs_b[0];
    c->n_objs = (uint32_t)tab.size(); c->n_work = (uint32_t)scene_work; c->n_inst_total = (uint32_t)scene_inst;
    { int rc = zr_update_table(c); if (rc) return rc; }      // (objects with updated instances: the parity-1 table, n_objs records)
    c->sky_object = sky ? (uint32_t)tab.size() - 1u : 0u;
    if (sky && !c->d_sky_keys) HIPCHK(c, c->ext.alloc(&c->d_sky_keys, (size_t)c->W * c->H));
    // A world update asked for the history to be carried (zr_ctx::history_remap): per kept draw the old work range and the new base; where
    // the instance count changed, the common prefix of instances.  The old planes are copied out first: ranges overlap when a base shifts
    // by less than a draw's length, in either direction, and make_work_pools releases the planes themselves.
    std::vector<ZrHistoryRange> ranges;
    uint64_t carried = 0;
    if (c->history_remap && old_work && c->d_visflag[0] && c->d_visflag[1] && c->d_sflag)
        for (const auto& o : c->objects) {
            const ZrObject& d = tab[o.draw];
            if (!o.work_valid || o.work_meshlets != d.n_meshlets) continue;
            const uint64_t count = (uint64_t)std::min(o.work_inst, d.n_inst) * d.n_meshlets;
            if (count == 0 || (uint64_t)o.work_base + count > old_work || (uint64_t)d.work_base + count > scene_work) continue;
            ranges.push_back({ d.work_base, o.work_base, (uint32_t)count, 0u });
            carried += count;
        }
    c->history_remap = false;
    std::sort(ranges.begin(), ranges.end(), [](const ZrHistoryRange& a, const ZrHistoryRange& b) { return a.new_base < b.new_base; });
    ZrOwn scratch;                      // (released when this returns, after the stream has drained)
    ZrHistoryCarry H = {};
    if (!ranges.empty()) {
        const size_t plane = ((size_t)old_work + 255u) & ~(size_t)255u;
        uint8_t* old = nullptr; ZrHistoryRange* d_ranges = nullptr;
        HIPCHK(c, scratch.alloc(&old, 3 * plane)); HIPCHK(c, upload(scratch, &d_ranges, ranges));
        const uint8_t* from[3] = { c->d_visflag[0], c->d_visflag[1], c->d_sflag };
        for (int k = 0; k < 3; ++k) { HIPCHK(c, hipMemcpyAsync(old + k * plane, from[k], old_work, hipMemcpyDeviceToDevice, c->stream)); H.src[k] = old + k * plane; }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        H.ranges = d_ranges; H.n_ranges = (uint32_t)ranges.size(); H.n_old = old_work; H.n_new = c->n_work;
    }
    if (c->n_work > c->work_capacity) { int rc = make_work_pools(c, c->n_work); if (rc) return rc; }
    c->any_images = c->mixed_images = false;
    for (const ZrObject& d : tab) for (int t = 0; t < 7; ++t) if (d.tex[t].data) c->any_images = true;
    for (const auto& o : c->objects) if (o.mixed_sizes) c->mixed_images = true;      // (the skydome's one image is sampled by itself)
    if (H.n_ranges) {
        // The marks and flags of the kept draws under their new numbers, stamp 0 and flag 1 everywhere else: vis_history, sflag_history,
        // vis_mark_prev, vis_cur and shadow_draws stay as they are, and so does the plan (per tile, not per work item) unless the pools
        // were re-made.  The camera lane reads the planes: the host waits for the carry.
        H.dst[0] = c->d_visflag[0]; H.dst[1] = c->d_visflag[1]; H.dst[2] = c->d_sflag;
        zr_launch_history_carry(H, c->stream);
        uint64_t moved[4] = { 0, 0, 0, 0 };      // the shadow flags' retest turn follows the items (zr_ctx::sflag_turn)
        for (const ZrHistoryRange& r : ranges) moved[(r.new_base - r.old_base) & 3u] += r.count;
        uint32_t d = 0;
        for (uint32_t k = 1; k < 4u; ++k) if (moved[k] > moved[d]) d = k;
        c->sflag_turn = (c->sflag_turn + 4u - d) & 3u;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        // work item numbering changed: last frame's visibility says nothing about this scene, and neither do its per-tile record counts
        // (the next frame counts before it draws: tri_raster) or the shadow flags
        zr_history_forgotten(c, ZR_HIST_VISIBILITY | ZR_HIST_PLAN | ZR_HIST_SHADOW_FLAGS);
        if (c->n_work) HIPCHK(c, hipMemsetAsync(c->d_sflag, 1, c->n_work, c->stream));      // shadow pass: everything is drawn in the first launch
    }
    c->history_items = carried;
    for (auto& o : c->objects) {        // the numbers the history knows the objects by from here on
        const ZrObject& d = tab[o.draw];
        o.work_base = d.work_base; o.work_inst = d.n_inst; o.work_meshlets = d.n_meshlets; o.work_valid = true;
    }
    zr_history_forgotten(c, ZR_HIST_LISTS);           // ... and neither do the passes' work lists
    zr_casters_changed(c);                            // ... nor the kept shadow map: new draw table, maybe new pools
    c->scene_dirty = false;
    return ZR_OK;
}

// ------------------------------------------------------------------------------------------------ skydome + background

extern "C" int zr_set_skydome(zr_ctx* c, const XkVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, const zr_image* tex)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        c->sky_mesh = ZrMesh(); c->sky_obj = ZrSceneObject(); c->sky_set = false; c->scene_dirty = true;      // (releasing the old ones)
        c->world_named[1] = false;
        if (!tex || !tex->rgba8) return ZR_OK;
        ARGCHK(c, v && idx && nv > 0 && ni > 0 && ni % 3 == 0);
        for (uint32_t i = 0; i < ni; ++i) if (idx[i] >= nv) return zr_fail(c, ZR_ERR_ARG, "index out of range");
        c->sky_mesh.v.assign(v, v + nv); c->sky_mesh.idx.assign(idx, idx + ni);
        ZrSceneObject& o = c->sky_obj;
        o.mesh = 0; o.instanced = false; o.n_inst = 1;
        for (int t = 0; t < 7; ++t) o.texel[t] = 0xFFFFFFFFu;
        o.bc_linear[0] = o.bc_linear[1] = o.bc_linear[2] = 1.0f;
        int rc = upload_image(c, o.mem, tex->rgba8, tex->width, tex->height, true, &o.d_tex[0], &o.tex_w[0], &o.tex_h[0], &o.tex_levels[0]);   // sRGB by default, ZE:5860
        if (rc) return rc;
        HIPCHK(c, o.mem.alloc(&o.d_inst, 1));
        zr_launch_instance_prep(nullptr, o.d_inst, 1, 0u, c->stream);
        HIPCHK(c, zr_sync_all(c));
        c->sky_set = true;
        return ZR_OK;
    });
}

extern "C" int zr_set_background(zr_ctx* c, const zr_image* tex)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        c->bg_mem.release(); c->d_bg = nullptr; c->bg_set = false; c->world_named[2] = false;
        zr_settle_forget(&c->lk.settle);      // (light_emit reads the image: a new one may lie where the old one lay)
        if (!tex || !tex->rgba8) return ZR_OK;
        int rc = upload_image(c, c->bg_mem, tex->rgba8, tex->width, tex->height, true, &c->d_bg, &c->bg_w, &c->bg_h, &c->bg_levels);
        if (rc) return rc;
        c->bg_set = true;
        return ZR_OK;
    });
}

extern "C" int zr_set_sky_flags(zr_ctx* c, int sky, int bg)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if ((sky != 0) != c->sky_enabled) c->scene_dirty = true;
        c->sky_enabled = sky != 0; c->bg_enabled = bg != 0;
        return ZR_OK;
    });
}

// ------------------------------------------------------------------------------------------------ cubemap

extern "C" int zr_set_cubemap(zr_ctx* c, const uint8_t* const faces[6], uint32_t dim)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        static const uint8_t grey[4] = { 127, 127, 127, 255 };
        if (!faces) dim = 1;
        ARGCHK(c, dim > 0 && dim <= 16384);
        if (faces) for (int f = 0; f < 6; ++f) ARGCHK(c, faces[f] != nullptr);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, zr_sync_all(c));
        c->cube_mem.release(); c->world_named[0] = false; c->cube_gen++;      // (what the lighting pass kept of the old texels is void)
        memset(&c->cube, 0, sizeof c->cube);
        uint32_t levels = 1; for (uint32_t d = dim; d > 1; d >>= 1) levels++;      // floor(log2(dim)) + 1, ZE:6887
        if (levels > 16) return zr_fail(c, ZR_ERR_ARG, "cubemap too large");
        std::vector<std::vector<uint8_t>> lv(levels);
        const size_t fsz = (size_t)dim * dim * 4;
        lv[0].resize(fsz * 6);
        for (int f = 0; f < 6; ++f) { if (faces) memcpy(lv[0].data() + fsz * f, faces[f], fsz); else memcpy(lv[0].data() + fsz * f, grey, 4); }
        uint32_t d = dim;
        for (uint32_t l = 1; l < levels; ++l) {        // RHIGenerateMipmaps: vkCmdBlitImage LINEAR from level l-1 (2x2 box, linear light)
            const uint32_t nd = d > 1 ? d >> 1 : 1;
            lv[l].resize((size_t)nd * nd * 4 * 6);
            for (int f = 0; f < 6; ++f) {
                const uint8_t* src = lv[l - 1].data() + (size_t)d * d * 4 * f;
                uint8_t* dst = lv[l].data() + (size_t)nd * nd * 4 * f;
                for (uint32_t y = 0; y < nd; ++y) for (uint32_t x = 0; x < nd; ++x) {
                    const uint32_t x0 = 2 * x, x1 = (2 * x + 1 < d) ? 2 * x + 1 : d - 1, y0 = 2 * y, y1 = (2 * y + 1 < d) ? 2 * y + 1 : d - 1;
                    const uint8_t* p00 = src + ((size_t)y0 * d + x0) * 4; const uint8_t* p10 = src + ((size_t)y0 * d + x1) * 4;
                    const uint8_t* p01 = src + ((size_t)y1 * d + x0) * 4; const uint8_t* p11 = src + ((size_t)y1 * d + x1) * 4;
                    for (int ch = 0; ch < 3; ++ch) {
                        const float a = (c->lut[p00[ch]] + c->lut[p10[ch]]) + (c->lut[p01[ch]] + c->lut[p11[ch]]);
                        dst[((size_t)y * nd + x) * 4 + ch] = srgb_encode8(a * 0.25f);
                    }
                    const uint32_t al = (uint32_t)p00[3] + p10[3] + p01[3] + p11[3];
                    dst[((size_t)y * nd + x) * 4 + 3] = (uint8_t)((al + 2) >> 2);
                }
            }
            d = nd;
        }
        for (uint32_t l = 0; l < levels; ++l) {
            uint8_t* p = nullptr;
            HIPCHK(c, upload(c->cube_mem, &p, lv[l]));
            c->cube.levels[l] = p;
        }
        c->cube_dim = dim; c->cube_levels = levels;
        c->view.LightsCount[3] = (int32_t)levels;       // CubemapMaxMips, ZE:4308
        c->view_dirty = true;
        return ZR_OK;
    });
}
