// Address arithmetic of the erase launch (mj_plan_set_erase), shared by k_erase (erase.hip) and its host twin mj_host_erase:
// which elements of an output's slot a box covers, as contiguous runs in the plan's layout, and where the element of a
// (C, height, width) block of values that goes to each of them lies.
//
// A slot is one ow x oh canvas of C components in one of the four layouts; a box is (x, y, w, h) inside it, x along the width.
//   layout                      runs of a box   elements per run   run r is
//   MJ_LAYOUT_ROWMAJOR          h               w * C              row y + r, pixels x .. x + w - 1, components interleaved
//   MJ_LAYOUT_PLANAR_ROWMAJOR   C * h           w                  component r / h, row y + r % h
//   MJ_LAYOUT_XMAJOR            w               h * C              column x + r, pixels y .. y + h - 1, components interleaved
//   MJ_LAYOUT_PLANAR_XMAJOR     C * w           h                  component r / w, column x + r % w
// Element e of a run belongs to pixel e / group along the run and to component comp + e % group (group: C interleaved, 1 planar).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace mj {

struct EraseCanvas {
    int32_t ow, oh, C, layout;
};

struct EraseRun {
    int64_t first;      // element offset of the run's first element inside the slot
    int64_t src;        // index, inside the box's (C, h, w) block, of the value of element 0
    int64_t src_cstep;  // ... from one component to the next inside a pixel (interleaved layouts)
    int32_t src_step;   // ... from one pixel of the run to the next
    int32_t len;        // elements
    int32_t group;      // elements per pixel along the run
    int32_t comp;       // the component of element 0
};

__host__ __device__ inline int erase_run_count(const EraseCanvas &k, int w, int h) {
    const int along = (k.layout & 1) ? h : w;           // row-major layouts: one run per row; x-major: one per column
    return k.layout >= 2 ? k.C * along : along;
}

// run r (0 .. erase_run_count - 1) of the box (x, y, w, h)
__host__ __device__ inline EraseRun erase_run(const EraseCanvas &k, int x, int y, int w, int h, int r) {
    const bool rows = (k.layout & 1) != 0, planar = k.layout >= 2;
    const int along = rows ? h : w;                     // runs per component plane
    const int c = planar ? r / along : 0, i = planar ? r - c * along : r;
    const int64_t plane = (int64_t)k.ow * k.oh, box = (int64_t)w * h;
    // the pixel the run starts at, counted along the layout's contiguous axis
    const int64_t pixel = rows ? (int64_t)(y + i) * k.ow + x : (int64_t)(x + i) * k.oh + y;
    EraseRun u;
    u.group = planar ? 1 : k.C;
    u.comp = c;
    u.len = (rows ? w : h) * u.group;
    u.first = planar ? c * plane + pixel : pixel * k.C;
    // the block is (C, h, w): a row of the box is contiguous in it, a column steps by w
    u.src = c * box + (rows ? (int64_t)i * w : (int64_t)i);
    u.src_step = rows ? 1 : w;
    u.src_cstep = box;
    return u;
}

// One box as the launch and the host twin take it: mj_erase_rect checked and resolved — the slot's first element, the constant as
// element bit patterns
struct DevEraseRect {
    int64_t slot_off;       // elements: where the output's slot starts in the array
    int64_t src_off;        // MJ_ERASE_VALUES: element offset of the box's (C, h, w) block in the values
    int32_t x, y, w, h;
    int32_t kind;           // MJ_ERASE_*
    uint32_t bits[3];       // MJ_ERASE_CONST: the element of each output component, in the low bytes
};
// One workgroup's work: runs run0 .. run0 + n_runs - 1 of box `rect`, dealt out to its wavefronts run by run
struct DevEraseJob {
    int32_t rect, run0, n_runs, pad;
};
struct EraseArgs {
    void *dst;                      // the array of slots
    const DevEraseRect *rects;
    const DevEraseJob *jobs;        // this launch's
    const void *values;
    EraseCanvas canvas;
    int32_t n_jobs;
};
// the job list of boxes order[0 .. n): every box's runs cut into jobs of about kEraseJobElements elements, at least four runs
// each (one per wavefront), appended to `jobs`
constexpr int kEraseJobElements = 8192;
template <class Jobs>
inline void erase_jobs(const EraseCanvas &k, const DevEraseRect *rects, const int32_t *order, int n, Jobs &jobs) {
    for (int i = 0; i < n; ++i) {
        const DevEraseRect &r = rects[order[i]];
        const int runs = erase_run_count(k, r.w, r.h), len = erase_run(k, r.x, r.y, r.w, r.h, 0).len;
        const int per = kEraseJobElements / len > 4 ? kEraseJobElements / len : 4;
        for (int r0 = 0; r0 < runs; r0 += per) jobs.push_back(DevEraseJob{order[i], r0, runs - r0 < per ? runs - r0 : per, 0});
    }
}
// esize: 1, 2 or 4 bytes per element
hipError_t launch_erase(hipStream_t stream, const EraseArgs &a, int esize);

// bytes per element of an MJ_DTYPE_* (0: none of them)
__host__ __device__ inline int erase_esize(int dtype) { return dtype == 0 ? 1 : dtype == 1 || dtype == 2 ? 2 : dtype == 3 ? 4 : 0; }

}  // namespace mj
