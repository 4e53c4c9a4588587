// zr_meshlet.cpp — the library's own meshlet clusteriser and bounds (host, load time).
//
// Replaces the ZeldaMeshlet tool's BuildMeshlets (Engine/ZeldaMeshlet/ZeldaMeshlet.cpp:132-172), which calls
// meshoptimizer (absent from the reference tree; submodule pin unrecoverable).  The partition itself never
// reaches a pixel (culling is conservative, the depth/visibility key carries the draw-order triangle id), so
// this is NOT a restatement of meshopt_buildMeshlets; it is a greedy adjacency clusteriser honouring the same
// contract: <= max_vertices unique vertices, <= max_triangles triangles, every triangle in exactly one
// meshlet, bounds that enclose, and a normal cone per meshoptimizer's published definition
// (cutoff = sqrt(1 - mindp^2), 1 when the cone is wider than ~84 degrees).
#include "zr_meshlet.h"
#include "zr_bounds.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

struct V3 { double x, y, z; };
inline V3 operator-(V3 a, V3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline V3 operator+(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline V3 operator*(V3 a, double s) { return { a.x * s, a.y * s, a.z * s }; }
inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 cross(V3 a, V3 b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
inline V3 pos(const XkVertex& v) { return { v.Position[0], v.Position[1], v.Position[2] }; }
typedef std::vector<std::vector<uint32_t>> Partition;       // triangle indices per meshlet, in emission order

}  // namespace

void zr_meshlet_bounds(const XkVertex* verts, const uint32_t* mv, uint32_t nv, const uint8_t* mt, uint32_t nt, XkMeshlet* out)
{
    // (the statement itself: zr_bounds.h, shared with the device's refit after a vertex update)
    zr_meshlet_bounds_of(verts, mv, nv, [mt](uint32_t t, uint32_t k) -> uint32_t { return mt[3u * t + k]; }, nt, out);
}

// Candidate 1: greedy growth over the vertex adjacency (what round 1 and 2 shipped).  Fills a cluster to the vertex limit and reseeds
// at the frontier; good on irregular and thin two-sided meshes, but leaves runts on regular ones.
static void cluster_greedy(const XkVertex* verts, uint32_t nv, const uint32_t* idx, uint32_t ni,
                           uint32_t max_vertices, uint32_t max_triangles, float cone_weight, Partition* out)
{
    const uint32_t nt = ni / 3;
    out->clear();

    // triangle centroid + unit normal
    std::vector<V3> cen(nt), nrm(nt);
    for (uint32_t t = 0; t < nt; ++t) {
        V3 a = pos(verts[idx[3 * t]]), b = pos(verts[idx[3 * t + 1]]), c = pos(verts[idx[3 * t + 2]]);
        cen[t] = (a + b + c) * (1.0 / 3.0);
        V3 n = cross(b - a, c - a); double l = std::sqrt(dot(n, n));
        nrm[t] = l > 0 ? n * (1.0 / l) : V3{ 0, 0, 0 };
    }
    // vertex -> triangle adjacency (CSR)
    std::vector<uint32_t> vstart(nv + 1, 0), vtri(ni);
    for (uint32_t i = 0; i < ni; ++i) vstart[idx[i] + 1]++;
    for (uint32_t v = 0; v < nv; ++v) vstart[v + 1] += vstart[v];
    { std::vector<uint32_t> fill(vstart.begin(), vstart.end() - 1);
      for (uint32_t i = 0; i < ni; ++i) vtri[fill[idx[i]]++] = i / 3; }

    std::vector<uint8_t> used(nt, 0);
    std::vector<uint8_t> vlocal(nv, 0xFF);
    std::vector<uint32_t> stamp(nt, 0xFFFFFFFFu);
    std::vector<uint32_t> cur_v; cur_v.reserve(max_vertices);
    std::vector<uint32_t> cur_t; cur_t.reserve(max_triangles);
    V3 csum = { 0, 0, 0 }, nsum = { 0, 0, 0 };
    uint32_t seed = 0, done = 0;

    auto flush = [&]() {
        if (cur_t.empty()) return;
        out->push_back(cur_t);
        for (uint32_t v : cur_v) vlocal[v] = 0xFF;
        cur_v.clear(); cur_t.clear(); csum = { 0, 0, 0 }; nsum = { 0, 0, 0 };
    };
    auto extra_of = [&](uint32_t t) {
        uint32_t a = idx[3 * t], b = idx[3 * t + 1], c = idx[3 * t + 2];
        uint32_t e = (vlocal[a] == 0xFF);
        if (b != a) e += (vlocal[b] == 0xFF);
        if (c != a && c != b) e += (vlocal[c] == 0xFF);
        return e;
    };
    auto add = [&](uint32_t t) {
        for (int k = 0; k < 3; ++k) {
            uint32_t v = idx[3 * t + k];
            if (vlocal[v] == 0xFF) { vlocal[v] = (uint8_t)cur_v.size(); cur_v.push_back(v); }
        }
        cur_t.push_back(t); used[t] = 1; done++;
        csum = csum + cen[t]; nsum = nsum + nrm[t];
    };

    // mean squared triangle "size" (centroid-to-vertex), used to price a new vertex against distance from the centroid
    double size2 = 0;
    for (uint32_t t = 0; t < nt; ++t) { V3 d = pos(verts[idx[3 * t]]) - cen[t]; size2 += dot(d, d); }
    size2 /= (double)nt;

    while (done < nt) {
        uint32_t best = 0xFFFFFFFFu; double best_score = 0;
        if (!cur_t.empty()) {
            const double inv = 1.0 / (double)cur_t.size();
            const V3 cc = csum * inv;
            double nl = std::sqrt(dot(nsum, nsum));
            const V3 na = nl > 0 ? nsum * (1.0 / nl) : V3{ 0, 0, 0 };
            const uint32_t mark = done;   // unique per step
            for (uint32_t v : cur_v)
                for (uint32_t k = vstart[v]; k < vstart[v + 1]; ++k) {
                    const uint32_t t = vtri[k];
                    if (used[t] || stamp[t] == mark) continue;
                    stamp[t] = mark;
                    // compact, cone-coherent growth: distance to the running centroid, widened by the normal deviation,
                    // plus a price per vertex the triangle would add (triangles closing a fan are nearly free)
                    const V3 d = cen[t] - cc;
                    const double score = dot(d, d) * (1.0 + (double)cone_weight * (1.0 - dot(nrm[t], na))) + size2 * (double)extra_of(t);
                    if (best == 0xFFFFFFFFu || score < best_score) { best = t; best_score = score; }
                }
        }
        if (best == 0xFFFFFFFFu) {          // no neighbour left: close the cluster and reseed
            flush();
            while (used[seed]) seed++;
            best = seed;
        } else if (cur_t.size() + 1 > max_triangles || cur_v.size() + extra_of(best) > max_vertices) {
            // full: close it and reseed next to it, at the frontier triangle with the fewest unused neighbours (keeps the
            // uncovered region convex-ish and avoids stranding islands of a few triangles)
            uint32_t pick = 0xFFFFFFFFu; uint32_t pick_live = 0xFFFFFFFFu;
            const uint32_t mark = done | 0x80000000u;
            for (uint32_t v : cur_v)
                for (uint32_t k = vstart[v]; k < vstart[v + 1]; ++k) {
                    const uint32_t t = vtri[k];
                    if (used[t] || stamp[t] == mark) continue;
                    stamp[t] = mark;
                    uint32_t live = 0;
                    for (int c3 = 0; c3 < 3; ++c3) { const uint32_t vv = idx[3 * t + c3]; for (uint32_t kk = vstart[vv]; kk < vstart[vv + 1]; ++kk) live += !used[vtri[kk]]; }
                    if (live < pick_live) { pick_live = live; pick = t; }
                }
            flush();
            best = pick != 0xFFFFFFFFu ? pick : best;
        }
        add(best);
    }
    flush();
}

// Candidate 2: slab x sector tiling.  Seen along an axis `a`, the mesh is cut into SLABS (bands of consecutive rows: the rows are the
// intervals between the distinct vertex levels along `a` when the mesh has few of them - a lathed or gridded mesh - and quantiles of the
// triangle centroids otherwise); every slab is swept in a second coordinate (the azimuth around `a`, or one of the two perpendicular
// directions) and cut into the least number n of pieces of EQUAL vertex weight that all respect the limits (a triangle weighs
// sum 1 / valence over its corners, i.e. its share of the vertices it brings); a dynamic programme over the slab boundaries picks the
// heights.  On a ring the sweep's starting point matters (cuts that fall on a column boundary save a row of vertices): every rotation
// within the first piece is tried.  Nothing is left over by construction: all pieces of a slab have the same weight.
// On the engine's 960-triangle sphere this finds 11 meshlets of 84-90 triangles (bands of 6 / 4 / 6 rows cut into 4 / 3 / 4 sectors;
// 10 is impossible: a pole fan costs a vertex per triangle); the greedy walk leaves 14 with runts of 3, 16, 29 and 43 triangles.
namespace {

struct TileCtx2 {
    const uint32_t* idx; uint32_t nt, nv, max_v, max_t;
    std::vector<uint32_t> stamp; uint32_t stamp_id = 0;
    std::vector<double> w;                 // vertex weight per triangle
    uint64_t work = 0, budget = 0;         // triangle visits spent / allowed
    std::vector<uint32_t> seq2, reach; std::vector<uint16_t> ref;      // chop_sweep's scratch (ref: per-vertex reference counts, all zero between calls)
    bool piece_ok(const uint32_t* t, size_t n)
    {
        if (n > max_t) return false;
        ++stamp_id; uint32_t cnt = 0;
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) { const uint32_t v = idx[3 * t[i] + k]; if (stamp[v] != stamp_id) { stamp[v] = stamp_id; if (++cnt > max_v) { work += i + 1; return false; } } }
        work += n;
        return true;
    }
    uint32_t count_verts(const uint32_t* t, size_t n)
    {
        ++stamp_id; uint32_t cnt = 0;
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) { const uint32_t v = idx[3 * t[i] + k]; if (stamp[v] != stamp_id) { stamp[v] = stamp_id; ++cnt; } }
        work += n;
        return cnt;
    }
};

// Cuts one sweep (a slab's triangles in sweep order; a ring when the sweep is an azimuth) into the LEAST number of consecutive pieces that
// respect the limits, and among those cuttings into the one whose smallest piece is largest (no runts).  reach[c] = the furthest end e
// such that seq[c, e) is a valid piece (two pointers with per-vertex reference counts; validity is monotone: a part of a valid piece is
// valid, so reach is non-decreasing).  The least count from a start is then the number of maximal jumps; the balance comes from a
// search on the smallest allowed piece length m (pieces of length in [m, reach]) and a forward pass that aims at equal shares of the
// rest.  On a ring every starting point of the doubled sequence is tried at O(pieces) apiece.
static void chop_sweep(TileCtx2& C, const std::vector<uint32_t>& seq_in, bool ring, uint32_t give_up_at, std::vector<std::vector<uint32_t>>* pieces)
{
    pieces->clear();
    const size_t L = seq_in.size();
    if (!L) return;
    const size_t L2 = ring ? 2 * L : L;
    std::vector<uint32_t>& seq = C.seq2; seq.resize(L2);
    for (size_t i = 0; i < L2; ++i) seq[i] = seq_in[i % L];
    std::vector<uint32_t>& reach = C.reach; reach.resize(L2 + 1);
    {   // two pointers
        std::vector<uint16_t>& ref = C.ref;
        uint32_t nverts = 0; size_t j = 0;
        auto corners = [&](uint32_t t, uint32_t* v) { v[0] = C.idx[3 * t]; v[1] = C.idx[3 * t + 1]; v[2] = C.idx[3 * t + 2]; };
        for (size_t c = 0; c < L2; ++c) {
            if (j < c) j = c;
            for (; j < L2 && j - c < C.max_t && j - c < L; ++j) {
                uint32_t v[3]; corners(seq[j], v);
                uint32_t add = (ref[v[0]] == 0) + (v[1] != v[0] && ref[v[1]] == 0) + (v[2] != v[0] && v[2] != v[1] && ref[v[2]] == 0);
                if (nverts + add > C.max_v) break;
                nverts += add; ++ref[v[0]]; ++ref[v[1]]; ++ref[v[2]];
            }
            reach[c] = (uint32_t)j;
            if (j > c) { uint32_t v[3]; corners(seq[c], v); for (int k = 0; k < 3; ++k) if (--ref[v[k]] == 0) --nverts; }
        }
        reach[L2] = (uint32_t)L2;
        C.work += 2 * L2;
    }
    // least number of pieces over the starting points
    const size_t n_start = ring ? L : 1;
    size_t best_n = (size_t)-1;
    std::vector<size_t> starts;
    for (size_t r = 0; r < n_start; ++r) {
        size_t c = r, n = 0; const size_t end = r + L;
        while (c < end && n <= best_n) { c = std::min<size_t>(reach[c], end); ++n; }
        if (c < end) continue;
        if (n < best_n) { best_n = n; starts.clear(); }
        if (n == best_n && starts.size() < 64) starts.push_back(r);
        C.work += n;
    }
    if (best_n == (size_t)-1 || best_n >= give_up_at) return;
    const size_t n = best_n;
    // among the starts with the least count: the one that admits the largest smallest piece
    auto feasible = [&](size_t r, size_t m) {
        size_t lo = r, hi = r; const size_t end = r + L;
        for (size_t k = 0; k < n; ++k) { lo += m; hi = std::min<size_t>(reach[hi], end); if (lo > hi) return false; }
        return hi == end && lo <= end;
    };
    size_t best_r = starts[0], best_m = 1;
    for (size_t r : starts) {
        size_t a = 1, b = L / n;                       // largest m with feasible(r, m); m = 1 is feasible (the maximal jumps)
        while (a < b) { const size_t mid = (a + b + 1) / 2; if (feasible(r, mid)) a = mid; else b = mid - 1; }
        if (a > best_m) { best_m = a; best_r = r; }
        C.work += n * 8;
    }
    // forward pass: aim every cut at an equal share of what is left, inside [c + m, reach[c]], and never so far left that the remaining
    // pieces could not reach the end even with maximal jumps
    for (size_t m = best_m; m >= 1; --m) {
        const size_t r = best_r, end = r + L;
        std::vector<size_t> cuts(1, r);
        bool ok = true;
        for (size_t k = 0; k + 1 < n && ok; ++k) {
            const size_t c = cuts.back(), left = n - k;
            size_t want = c + (end - c + left - 1) / left;
            size_t lo = c + m, hi = std::min<size_t>(reach[c], end - (left - 1) * 1);
            if (lo > hi) { ok = false; break; }
            size_t nc = std::min(std::max(want, lo), hi);
            auto covers = [&](size_t from) { size_t q = from; for (size_t j = 0; j + 1 < left && q < end; ++j) q = std::min<size_t>(reach[q], end); return q >= end; };
            while (nc < hi && !covers(nc)) ++nc;
            if (!covers(nc)) { ok = false; break; }
            cuts.push_back(nc);
        }
        if (ok && reach[cuts.back()] < end) ok = false;
        if (!ok) continue;
        cuts.push_back(end);
        for (size_t k = 0; k + 1 < cuts.size(); ++k)
            if (cuts[k + 1] > cuts[k]) pieces->emplace_back(seq.begin() + (long)cuts[k], seq.begin() + (long)cuts[k + 1]);
        return;
    }
}

// mode 0: sweep by azimuth around the axis; 1 / 2: by the first / second perpendicular direction.  false: gave up (budget, or no better than `limit`)
static bool tile_slabs(TileCtx2& C, const std::vector<V3>& cen, const std::vector<V3>& vpos, V3 origin, V3 a, int mode, size_t limit, Partition* out)
{
    const double al = std::sqrt(dot(a, a));
    if (!(al > 0)) return false;
    a = a * (1.0 / al);
    const V3 t = std::fabs(a.x) < 0.9 ? V3{ 1, 0, 0 } : V3{ 0, 1, 0 };
    V3 e1 = cross(a, t); e1 = e1 * (1.0 / std::sqrt(dot(e1, e1)));
    const V3 e2 = cross(a, e1);
    const uint32_t nt = C.nt;
    // rows
    std::vector<double> ucen(nt);
    double umin = 1e300, umax = -1e300;
    for (const V3& p : vpos) { const double u = dot(p, a); umin = std::min(umin, u); umax = std::max(umax, u); }
    for (uint32_t i = 0; i < nt; ++i) ucen[i] = dot(cen[i], a);
    const double range = umax - umin;
    std::vector<uint32_t> row(nt, 0);
    uint32_t R = 1;
    if (range > 0) {
        std::vector<double> lv(vpos.size());
        for (size_t i = 0; i < vpos.size(); ++i) lv[i] = dot(vpos[i], a);
        std::sort(lv.begin(), lv.end());
        std::vector<double> levels;
        for (double u : lv) if (levels.empty() || u - levels.back() > 1e-5 * range) levels.push_back(u);
        if (levels.size() >= 2 && levels.size() <= 513) {              // a structured mesh: rows between consecutive vertex levels
            R = (uint32_t)levels.size() - 1;
            for (uint32_t i = 0; i < nt; ++i) {
                const size_t k = (size_t)(std::upper_bound(levels.begin(), levels.end(), ucen[i]) - levels.begin());
                row[i] = (uint32_t)std::min<size_t>(k ? k - 1 : 0, R - 1);
            }
        } else {                                                       // quantile slabs of the centroids
            R = (uint32_t)std::min<size_t>(96, std::max<size_t>(1, nt / 16));
            std::vector<double> su(ucen); std::sort(su.begin(), su.end());
            std::vector<double> q;
            for (uint32_t k = 1; k < R; ++k) q.push_back(su[(size_t)((uint64_t)nt * k / R)]);
            for (uint32_t i = 0; i < nt; ++i) row[i] = (uint32_t)(std::upper_bound(q.begin(), q.end(), ucen[i]) - q.begin());
        }
    }
    std::vector<std::vector<uint32_t>> by_row(R);
    for (uint32_t i = 0; i < nt; ++i) by_row[row[i]].push_back(i);
    std::vector<double> key(nt);
    for (uint32_t i = 0; i < nt; ++i) {
        const V3 d = cen[i] - origin;
        key[i] = mode == 0 ? std::atan2(dot(d, e2), dot(d, e1)) : (mode == 1 ? dot(d, e1) : dot(d, e2));
    }
    const uint32_t Hmax = 16;
    std::vector<size_t> best(R + 1, (size_t)-1);
    std::vector<uint32_t> from(R + 1, 0);
    std::vector<std::vector<std::vector<uint32_t>>> slab_pieces(R + 1);       // pieces of the last slab of the best tiling ending at row b
    best[0] = 0;
    std::vector<uint32_t> seq;
    std::vector<std::vector<uint32_t>> pcs;
    for (uint32_t b = 1; b <= R; ++b) {
        for (uint32_t a0 = b > Hmax ? b - Hmax : 0; a0 < b; ++a0) {
            if (best[a0] == (size_t)-1) continue;
            seq.clear();
            for (uint32_t r = a0; r < b; ++r) seq.insert(seq.end(), by_row[r].begin(), by_row[r].end());
            if (seq.empty()) { if (best[a0] < best[b]) { best[b] = best[a0]; from[b] = a0; slab_pieces[b].clear(); } continue; }
            if ((uint64_t)seq.size() > 64ull * C.max_t * 16ull) continue;                 // taller than any useful slab
            std::stable_sort(seq.begin(), seq.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
            // how many pieces may this slab take at most to still beat what we have?
            const size_t room = std::min(best[b] == (size_t)-1 ? (size_t)-1 : best[b] - best[a0], limit > best[a0] ? limit - best[a0] : 0);
            if (room == 0) continue;
            chop_sweep(C, seq, mode == 0, (uint32_t)std::min<size_t>(room, 0xFFFFFFFFu), &pcs);
            if (C.work > C.budget) return false;
            if (pcs.empty()) continue;
            if (best[a0] + pcs.size() < best[b]) { best[b] = best[a0] + pcs.size(); from[b] = a0; slab_pieces[b] = pcs; }
        }
    }
    if (best[R] == (size_t)-1 || best[R] >= limit) return false;
    out->clear();
    std::vector<uint32_t> ends;
    for (uint32_t b = R; b > 0; b = from[b]) ends.push_back(b);
    for (size_t i = ends.size(); i-- > 0;)
        for (auto& p : slab_pieces[ends[i]]) out->push_back(p);
    return true;
}

}  // namespace

void zr_build_meshlets(const XkVertex* verts, uint32_t nv, const uint32_t* idx, uint32_t ni,
                       uint32_t max_vertices, uint32_t max_triangles, float cone_weight, ZrMeshletSet* out)
{
    const uint32_t nt = ni / 3;
    out->meshlets.clear(); out->mverts.clear(); out->mtris.clear(); out->tri_order.clear();
    if (nt == 0) return;
    Partition best;
    cluster_greedy(verts, nv, idx, ni, max_vertices, max_triangles, cone_weight, &best);

    // the tilings: only worth trying when the greedy result is above the counting bound, and only on finite geometry
    bool finite = true;
    for (uint32_t i = 0; i < nv && finite; ++i) for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(verts[i].Position[k]);
    std::vector<uint32_t> used_v(nv, 0); uint32_t n_used = 0;
    for (uint32_t i = 0; i < ni; ++i) if (!used_v[idx[i]]++) ++n_used;
    const size_t lower = std::max<size_t>((nt + max_triangles - 1) / max_triangles, (n_used + max_vertices - 1) / max_vertices);
    if (finite && best.size() > lower && max_vertices >= 8 && max_triangles >= 8) {
        TileCtx2 C; C.idx = idx; C.nt = nt; C.nv = nv; C.max_v = max_vertices; C.max_t = max_triangles;
        C.stamp.assign(nv, 0); C.w.resize(nt); C.ref.assign(nv, 0);
        for (uint32_t t = 0; t < nt; ++t) { double w = 0; for (int k = 0; k < 3; ++k) w += 1.0 / (double)used_v[idx[3 * t + k]]; C.w[t] = w; }
        C.budget = 400ull * 1000 * 1000 + 2000ull * nt;             // triangle visits: a second or two at load time, then the best so far stands
        std::vector<V3> cen(nt), vpos(nv);
        for (uint32_t i = 0; i < nv; ++i) vpos[i] = pos(verts[i]);
        V3 origin = { 0, 0, 0 };
        for (uint32_t t = 0; t < nt; ++t) { cen[t] = (vpos[idx[3 * t]] + vpos[idx[3 * t + 1]] + vpos[idx[3 * t + 2]]) * (1.0 / 3.0); origin = origin + cen[t]; }
        origin = origin * (1.0 / (double)nt);
        // axes: the principal axes of the centroids (Jacobi sweeps on the 3 x 3 covariance), then the coordinate axes
        double A[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
        for (uint32_t t = 0; t < nt; ++t) {
            const V3 d = cen[t] - origin; const double e[3] = { d.x, d.y, d.z };
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] += e[i] * e[j];
        }
        double Vv[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
        for (int sweep = 0; sweep < 24; ++sweep)
            for (int p = 0; p < 3; ++p) for (int q = p + 1; q < 3; ++q) {
                if (std::fabs(A[p][q]) < 1e-300) continue;
                const double th = 0.5 * std::atan2(2.0 * A[p][q], A[q][q] - A[p][p]), c = std::cos(th), s = std::sin(th);
                for (int k = 0; k < 3; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
                for (int k = 0; k < 3; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
                for (int k = 0; k < 3; ++k) { const double x = Vv[k][p], y = Vv[k][q]; Vv[k][p] = c * x - s * y; Vv[k][q] = s * x + c * y; }
            }
        std::vector<V3> axes = { { 0, 0, 1 }, { 1, 0, 0 }, { 0, 1, 0 } };
        for (int k = 0; k < 3; ++k) {
            const V3 e = { Vv[0][k], Vv[1][k], Vv[2][k] };
            bool dup = false;
            for (const V3& x : axes) if (std::fabs(dot(x, e)) > 0.9999) dup = true;
            if (!dup && std::isfinite(e.x + e.y + e.z) && dot(e, e) > 0.5) axes.push_back(e);
        }
        Partition cand;
        for (const V3& ax : axes)
            for (int mode = 0; mode < 3; ++mode) {
                if (best.size() <= lower || C.work > C.budget) break;
                if (tile_slabs(C, cen, vpos, origin, ax, mode, best.size(), &cand) && cand.size() < best.size()) best.swap(cand);
            }
    }

    // emit: meshlets in partition order, triangles in sweep order; vertices in first-use order
    std::vector<uint8_t> vlocal(nv, 0xFF);
    std::vector<uint32_t> cur_v;
    uint32_t tri_base = 0;
    for (const std::vector<uint32_t>& piece : best) {
        if (piece.empty()) continue;
        cur_v.clear();
        XkMeshlet m; std::memset(&m, 0, sizeof m);
        m.VertexOffset = (uint32_t)out->mverts.size(); m.TriangleOffset = (uint32_t)out->mtris.size();
        m.TriangleCount = (uint32_t)piece.size(); m.BindlessContext = tri_base;
        for (uint32_t t : piece) {
            for (int k = 0; k < 3; ++k) {
                const uint32_t v = idx[3 * t + k];
                if (vlocal[v] == 0xFF) { vlocal[v] = (uint8_t)cur_v.size(); cur_v.push_back(v); }
                out->mtris.push_back(vlocal[v]);
            }
            out->tri_order.push_back(t);
        }
        m.VertexCount = (uint32_t)cur_v.size();
        for (uint32_t v : cur_v) { out->mverts.push_back(v); vlocal[v] = 0xFF; }
        zr_meshlet_bounds(verts, out->mverts.data() + m.VertexOffset, m.VertexCount, out->mtris.data() + m.TriangleOffset, m.TriangleCount, &m);
        out->meshlets.push_back(m);
        tri_base += m.TriangleCount;
    }
}
