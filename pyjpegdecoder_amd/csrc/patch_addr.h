// The host side of the patchify launch (mj_patchify; tools/patch_model.py), shared by the launch's set-up (patch.hip), the kernel,
// the host twin mj_host_patchify and mj_host_patchify_count: where an element of a source's window lands in a token row, and the
// output cut into the jobs k_patchify and the host twin walk.
//
// A source slot is one sw x sh canvas of C components in MJ_LAYOUT_* `layout`.  Source k's window (x, y, w, h) is cut into P x P
// patches, gh = h / P by gw = w / P of them; patch (py, px) is token row
//     row0[k] + ((py / m) * (gw / m) + px / m) * m * m + (py % m) * m + px % m
// of D = C * t * P * P elements (row0[k]: the tokens of the sources before, or k * length in the padded form), element
//     chw:  ((c * t + r) * P + j) * P + i      for r in 0 .. t - 1          hwc:  (j * P + i) * C + c
// being pixel (px * P + i, py * P + j)'s component c.
//
// So within one source the tokens of one MERGE BAND — m patch rows, m * P pixel lines — are contiguous in the output, and so is
// any run of whole merge blocks (m x m patches, m * m tokens) inside a band.  A JOB is (source, band, run of merge blocks): its
// source is a rectangle of m * P lines by count * m * P pixels, its destination ONE contiguous range of count * m * m * D
// elements, at most kPatchJobBytes of them unless one merge block alone is more (kPatchBlockBytes at the most: refused beyond).
// In the padded form the rows behind a source's last token are fill jobs (src < 0) of zero elements.  The jobs partition the
// destination exactly.  Every offset is 64 bits wide.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include <hip/hip_runtime.h>

namespace mj {

constexpr int kPatchMaxPatch = 64, kPatchMaxMerge = 8, kPatchMaxRepeat = 4;
constexpr int kPatchBlockBytes = 65536;             // a merge block's most: the least a job holds
// What a job's destination range holds unless one block is more.  32 KiB lets four workgroups share a CU's LDS, 64 KiB two:
// that is the reason for the value; the two are not measured against each other.
constexpr int kPatchJobBytes = 32768;
constexpr int kPatchLdsSlack = 16;                  // the LDS image starts at the destination's address mod 16

// mj_patch_window, field for field (patch.hip asserts the size)
struct PatchWindow {
    int32_t x, y, w, h;
};
struct PatchGeom {
    int32_t sw, sh, C, layout;
    int32_t P, m, t, hwc;
    int32_t length;         // 0: packed
};

// One workgroup's work.  A copy job: `count` merge blocks of one band; a fill job (src < 0): `count` elements of zero.
struct DevPatchJob {
    int64_t dst;            // element offset of the job's range in the destination array
    int64_t src;            // element offset, in the source array, of component 0 of the rectangle's top-left pixel; below 0: fill
    int32_t count;
    int32_t pad_;
};
struct PatchArgs {
    const void *src;
    void *dst;
    const DevPatchJob *jobs;
    int64_t s_c, s_line;    // source elements from one component plane to the next (planar), from one line to the next
    uint64_t mulP, mulm;    // patch_div's multipliers for P and m
    int32_t n_jobs;
    int32_t C, P, m, t, D, mP;
    int32_t rows, planar;   // the contiguous axis is x; one plane per component
    int32_t cs;             // a token's element stride per component
    int32_t as, xs;         // ... per pixel along a line (within a patch), per pixel across the lines
    int32_t tok_step, tok_wrap;     // tokens from one patch to the next along a line, and more where that leaves a merge block
    int32_t tok_across;             // tokens from one patch to the next across the lines
};

// x / d as the high word of x * (2^32 / d + 1): exact while x * d < 2^32 — here x < 2^18 (an element of a line) and d <= 64
inline uint64_t patch_div_mul(int d) { return (((uint64_t)1 << 32) / (uint64_t)d) + 1; }
__host__ __device__ inline uint32_t patch_div(uint32_t x, uint64_t mul) { return (uint32_t)(((uint64_t)x * mul) >> 32); }

inline int patch_D(const PatchGeom &g) { return g.C * g.t * g.P * g.P; }

// `a` filled in but for src, dst, jobs and n_jobs
inline void patch_args(const PatchGeom &g, PatchArgs *a) {
    a->rows = (g.layout & 1) != 0;
    a->planar = g.layout >= 2;
    const int group = a->planar ? 1 : g.C;
    a->s_c = a->planar ? (int64_t)g.sw * g.sh : 1;
    a->s_line = (int64_t)(a->rows ? g.sw : g.sh) * group;
    a->mulP = patch_div_mul(g.P); a->mulm = patch_div_mul(g.m);
    a->C = g.C; a->P = g.P; a->m = g.m; a->t = g.t; a->D = patch_D(g); a->mP = g.m * g.P;
    a->cs = g.hwc ? 1 : g.t * g.P * g.P;
    const int is = g.hwc ? g.C : 1, js = g.hwc ? g.P * g.C : g.P;      // a token's strides per pixel along x and along y
    a->as = a->rows ? is : js; a->xs = a->rows ? js : is;
    a->tok_step = a->rows ? 1 : g.m; a->tok_wrap = a->rows ? g.m * g.m - g.m : 0;
    a->tok_across = a->rows ? g.m : 1;
}

// Where component c of pixel (xx, yy) of a job's rectangle lands in the job's range, repeat 0 (the others follow P * P apart)
__host__ __device__ inline int32_t patch_index(const PatchArgs &a, int c, int yy, int xx) {
    const int blk = xx / a.mP, ix = (xx % a.mP) / a.P, i = xx % a.P, iy = yy / a.P, j = yy % a.P;
    const int is = a.rows ? a.as : a.xs, js = a.rows ? a.xs : a.as;
    return ((blk * a.m + iy) * a.m + ix) * a.D + c * a.cs + j * js + i * is;
}

// whole canvases for windows == nullptr
inline PatchWindow patch_window(const PatchGeom &g, const PatchWindow *windows, int k) {
    return windows ? windows[k] : PatchWindow{0, 0, g.sw, g.sh};
}

// the rows of the output (checked geometry): packed, the tokens of all sources; padded, n_sources * length
inline int64_t patch_rows(const PatchGeom &g, int n_sources, const PatchWindow *windows) {
    if (g.length) return (int64_t)n_sources * g.length;
    int64_t rows = 0;
    for (int k = 0; k < n_sources; ++k) {
        const PatchWindow w = patch_window(g, windows, k);
        rows += (int64_t)(w.h / g.P) * (w.w / g.P);
    }
    return rows;
}

// the jobs of the launch, appended to `jobs`, in destination order; esize: bytes per element
inline void patch_jobs(const PatchGeom &g, int esize, int n_sources, const PatchWindow *windows, std::vector<DevPatchJob> &jobs) {
    const bool rows = (g.layout & 1) != 0, planar = g.layout >= 2;
    const int group = planar ? 1 : g.C;
    const int64_t D = patch_D(g), mP = (int64_t)g.m * g.P, slot = (int64_t)g.sw * g.sh * g.C;
    const int64_t s_x = rows ? group : (int64_t)g.sh * group, s_y = rows ? (int64_t)g.sw * group : group;
    const int64_t block = (int64_t)g.m * g.m * D;                        // elements of a merge block
    const int per = (int)std::max<int64_t>(1, kPatchJobBytes / (block * esize));
    const int64_t fill = kPatchJobBytes / esize;
    int64_t row0 = 0;
    for (int k = 0; k < n_sources; ++k) {
        const PatchWindow w = patch_window(g, windows, k);
        const int bands = (int)(w.h / mP), across = (int)(w.w / mP);
        if (g.length) row0 = (int64_t)k * g.length;
        for (int b = 0; b < bands; ++b)
            for (int x0 = 0; x0 < across; x0 += per) {
                DevPatchJob j;
                j.dst = (row0 + ((int64_t)b * across + x0) * g.m * g.m) * D;
                j.src = (int64_t)k * slot + (w.y + b * mP) * s_y + (w.x + x0 * mP) * s_x;
                j.count = std::min(per, across - x0);
                j.pad_ = 0;
                jobs.push_back(j);
            }
        const int64_t tokens = (int64_t)bands * across * g.m * g.m;
        if (g.length) {
            const int64_t end = (row0 + g.length) * D;
            for (int64_t e = (row0 + tokens) * D; e < end; e += fill) jobs.push_back(DevPatchJob{e, -1, (int32_t)std::min(fill, end - e), 0});
        } else {
            row0 += tokens;
        }
    }
}

// the most LDS a job of the launch needs: its range and the slack
inline size_t patch_lds_bytes(const PatchGeom &g, int esize) {
    const int64_t block = (int64_t)g.m * g.m * patch_D(g) * esize;
    return (size_t)(std::max<int64_t>(1, kPatchJobBytes / block) * block) + kPatchLdsSlack;
}

// esize: 1, 2 or 4 bytes per element; lds: patch_lds_bytes
hipError_t launch_patchify(hipStream_t stream, const PatchArgs &a, int esize, size_t lds);

}  // namespace mj
