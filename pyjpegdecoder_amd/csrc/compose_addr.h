// The host side of the compose launch (mj_compose; tools/compose_model.py), shared by the launch's set-up (compose.hip), its host
// twin mj_host_compose and mj_host_compose_resolve: an output's tiles resolved into DISJOINT rectangles that partition its canvas
// exactly, and the rectangles cut into the jobs k_compose and the host twin walk.  "A later tile wins" is decided here, once.
//
// A source slot is one sw x sh canvas, a destination slot one dw x dh canvas, both of C components in the same layout.  A tile
// pastes the window (sx, sy, w, h) of source slot `source` with its top-left corner at (dx, dy) of destination slot `output`,
// clipped to the canvas; what no tile covers is fill.
//
// LINES are the layout's contiguous runs (erase_addr.h, mix_rule.h); for a rectangle (x, y, w, h):
//   layout                      lines     elements per line   a line is
//   MJ_LAYOUT_ROWMAJOR          h         w * C               a row of the rectangle, components interleaved
//   MJ_LAYOUT_PLANAR_ROWMAJOR   C * h     w                   a row of one component plane
//   MJ_LAYOUT_XMAJOR            w         h * C               a column of the rectangle, components interleaved
//   MJ_LAYOUT_PLANAR_XMAJOR     C * w     h                   a column of one component plane
// Line l of a rectangle (of one of its planes) starts `l * line stride` elements behind its first line, in the destination and in
// the source alike — each with its own canvas's stride —, so a job carries the element offsets of its first line and the kernel
// forms a line's two addresses with one multiply-add each.  Every offset is 64 bits wide: 1024 tiles of 320 x 320 x 3 float32
// are 1.2 GB.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

namespace mj {

constexpr int kComposeMaxTiles = 64;                // tiles of one output
constexpr int kComposeMaxOffset = 1 << 20;          // |dx|, |dy| stay below it

struct ComposeGeom {
    int32_t sw, sh;         // a source canvas
    int32_t dw, dh;         // a destination canvas
    int32_t C, layout;
};
// mj_compose_tile / mj_compose_rect, field for field (compose.hip asserts the sizes)
struct ComposeTile {
    int32_t output, source, sx, sy, w, h, dx, dy;
};
struct ComposeRect {
    int32_t output, x, y, w, h;
    int32_t source;         // the source slot, or -1: fill
    int32_t sx, sy;         // where (x, y) lies on the source canvas
};

// One workgroup's work: `nlines` lines of `len` elements of one rectangle (of one component plane of it, in the planar layouts).
// P = 1 << shift lanes share a line, 256 / P lines are under way at a time.
struct DevComposeJob {
    int64_t dst;            // element offset, in the destination array, of the first line's first element
    int64_t src;            // ... in the source array; below 0: fill
    int32_t len, nlines;
    int32_t shift;
    int32_t comp;           // the component of the plane (planar layouts); 0 in the interleaved ones, where an element's is e % C
};
struct ComposeArgs {
    const void *src;
    void *dst;
    const DevComposeJob *jobs;
    int64_t dst_stride, src_stride;     // elements from one line to the next
    int32_t n_jobs, C3;                 // C3: three interleaved components (the fill pattern has a phase)
    uint32_t fill[3];
};
constexpr int kComposeJobBytes = 32768;             // about what a job writes
constexpr int kComposeUnroll = 4;                   // lines per lane and round

inline int64_t compose_slot_elems(int w, int h, int C) { return (int64_t)w * h * C; }

// The tiles of ONE output, in paste order, into rectangles appended to `out`: the coordinates of the clipped tile boxes are
// compressed, every cell gets its owner — the last tile that covers it, or fill —, cells of one owner are merged along the
// layout's contiguous axis and the strips that result, where they agree in extent and owner, across it.  At most
// (2 n + 1)^2 rectangles for n tiles (compose_rect_bound).
inline int64_t compose_rect_bound(int64_t n_tiles) { return (2 * n_tiles + 1) * (2 * n_tiles + 1); }

inline void compose_resolve_output(const ComposeGeom &g, int output, const ComposeTile *tiles, int n, std::vector<ComposeRect> &out) {
    const bool rows = (g.layout & 1) != 0;
    // in (a, b) coordinates: a along the contiguous axis, b across it
    const int A = rows ? g.dw : g.dh, Bn = rows ? g.dh : g.dw;
    struct Box { int a0, a1, b0, b1, tile; };
    std::vector<Box> boxes;
    std::vector<int> as{0, A}, bs{0, Bn};
    for (int t = 0; t < n; ++t) {
        const ComposeTile &q = tiles[t];
        const int x0 = std::max(q.dx, 0), y0 = std::max(q.dy, 0);
        const int x1 = (int)std::min<int64_t>((int64_t)q.dx + q.w, g.dw), y1 = (int)std::min<int64_t>((int64_t)q.dy + q.h, g.dh);
        if (x0 >= x1 || y0 >= y1) continue;             // (wholly outside: nothing is pasted)
        const Box b = rows ? Box{x0, x1, y0, y1, t} : Box{y0, y1, x0, x1, t};
        boxes.push_back(b);
        as.push_back(b.a0); as.push_back(b.a1); bs.push_back(b.b0); bs.push_back(b.b1);
    }
    std::sort(as.begin(), as.end()); as.erase(std::unique(as.begin(), as.end()), as.end());
    std::sort(bs.begin(), bs.end()); bs.erase(std::unique(bs.begin(), bs.end()), bs.end());
    const int na = (int)as.size() - 1, nb = (int)bs.size() - 1;
    std::vector<int> owner((size_t)na * nb, -1);
    for (const Box &b : boxes) {                        // (in paste order: a later tile overwrites)
        const int ia0 = (int)(std::lower_bound(as.begin(), as.end(), b.a0) - as.begin()), ia1 = (int)(std::lower_bound(as.begin(), as.end(), b.a1) - as.begin());
        const int ib0 = (int)(std::lower_bound(bs.begin(), bs.end(), b.b0) - bs.begin()), ib1 = (int)(std::lower_bound(bs.begin(), bs.end(), b.b1) - bs.begin());
        for (int j = ib0; j < ib1; ++j)
            for (int i = ia0; i < ia1; ++i) owner[(size_t)j * na + i] = b.tile;
    }
    struct Strip { int a0, a1, b0, b1, tile; };
    std::vector<Strip> open, next;
    auto emit = [&](const Strip &s) {
        ComposeRect r;
        r.output = output;
        r.x = rows ? s.a0 : s.b0; r.y = rows ? s.b0 : s.a0;
        r.w = rows ? s.a1 - s.a0 : s.b1 - s.b0; r.h = rows ? s.b1 - s.b0 : s.a1 - s.a0;
        r.source = -1; r.sx = r.sy = 0;
        if (s.tile >= 0) {
            const ComposeTile &q = tiles[s.tile];
            r.source = q.source; r.sx = q.sx + (r.x - q.dx); r.sy = q.sy + (r.y - q.dy);
        }
        out.push_back(r);
    };
    for (int j = 0; j < nb; ++j) {
        next.clear();
        for (int i = 0; i < na;) {                      // along the contiguous axis
            int e = i + 1;
            while (e < na && owner[(size_t)j * na + e] == owner[(size_t)j * na + i]) ++e;
            next.push_back(Strip{as[i], as[e], bs[j], bs[j + 1], owner[(size_t)j * na + i]});
            i = e;
        }
        for (const Strip &o : open) {                   // across it: a strip of the band before goes on, or is a rectangle
            bool on = false;
            for (Strip &s : next)
                if (s.a0 == o.a0 && s.a1 == o.a1 && s.tile == o.tile && s.b0 == o.b1) { s.b0 = o.b0; on = true; break; }
            if (!on) emit(o);
        }
        open.swap(next);
    }
    for (const Strip &o : open) emit(o);
}

// the jobs of one rectangle, appended to `jobs`: per component plane (one in the interleaved layouts) its lines in pieces of
// about kComposeJobBytes; esize: bytes per element
inline void compose_jobs(const ComposeGeom &g, int esize, const ComposeRect &r, std::vector<DevComposeJob> &jobs) {
    const bool rows = (g.layout & 1) != 0, planar = g.layout >= 2;
    const int group = planar ? 1 : g.C, planes = planar ? g.C : 1;
    const int64_t dstride = (int64_t)(rows ? g.dw : g.dh) * group, sstride = (int64_t)(rows ? g.sw : g.sh) * group;
    const int len = (rows ? r.w : r.h) * group, lines = rows ? r.h : r.w;
    const int64_t line_bytes = (int64_t)len * esize;
    // the lanes of a line: one per 16 bytes, and for a short line one per element of a head or tail — a power of two up to 256
    const int64_t want = std::max<int64_t>((line_bytes + 15) / 16, std::min<int64_t>(len, 16 / esize));
    int shift = 0;
    while (shift < 8 && ((int64_t)1 << shift) < want) ++shift;
    // (a multiple of the lines a workgroup has under way at a time: kComposeUnroll rounds of 256 >> shift)
    const int round = (256 >> shift) * kComposeUnroll;
    const int per = (int)((std::max<int64_t>(1, kComposeJobBytes / line_bytes) + round - 1) / round * round);
    for (int c = 0; c < planes; ++c) {
        const int64_t d0 = (int64_t)r.output * compose_slot_elems(g.dw, g.dh, g.C) + (int64_t)c * g.dw * g.dh +
                           (int64_t)(rows ? r.y : r.x) * dstride + (int64_t)(rows ? r.x : r.y) * group;
        const int64_t s0 = r.source < 0 ? -1
                                        : (int64_t)r.source * compose_slot_elems(g.sw, g.sh, g.C) + (int64_t)c * g.sw * g.sh +
                                              (int64_t)(rows ? r.sy : r.sx) * sstride + (int64_t)(rows ? r.sx : r.sy) * group;
        for (int l0 = 0; l0 < lines; l0 += per) {
            DevComposeJob j;
            j.dst = d0 + (int64_t)l0 * dstride;
            j.src = s0 < 0 ? -1 : s0 + (int64_t)l0 * sstride;
            j.len = len; j.nlines = std::min(per, lines - l0);
            j.shift = shift; j.comp = c;
            jobs.push_back(j);
        }
    }
}

// `a` filled in but for src, dst and jobs
inline void compose_args(const ComposeGeom &g, const uint32_t fill[3], ComposeArgs *a) {
    const bool rows = (g.layout & 1) != 0;
    const int group = g.layout >= 2 ? 1 : g.C;
    a->dst_stride = (int64_t)(rows ? g.dw : g.dh) * group;
    a->src_stride = (int64_t)(rows ? g.sw : g.sh) * group;
    a->C3 = group == 3;
    for (int c = 0; c < 3; ++c) a->fill[c] = fill[c < g.C ? c : 0];
}

// esize: 1, 2 or 4 bytes per element
hipError_t launch_compose(hipStream_t stream, const ComposeArgs &a, int esize);

}  // namespace mj
