// Erase (mj_plan_set_erase; tools/erase_model.py): boxes of the finished outputs overwritten with constants or with the caller's
// values — torchvision's F.erase, img[..., i:i+h, j:j+w] = v, on the array the plan's last launch has stored.  The kernel, its
// launch, the call that puts boxes on a plan, the launches of an execute, and the host twin.  The address arithmetic is
// erase_addr.h's, one set of functions for the kernel and the twin.
#include <math.h>

#include "plan.h"

namespace mj {

typedef unsigned int mj_eu32x4 __attribute__((ext_vector_type(4)));
template <int ES> struct EraseElem;
template <> struct EraseElem<1> { typedef uint8_t T; };
template <> struct EraseElem<2> { typedef uint16_t T; };
template <> struct EraseElem<4> { typedef uint32_t T; };

// One workgroup per job, one wavefront per run of it in turn.  A run is contiguous: the elements in front of its first 16-byte
// boundary and behind its last one are stored one by one, the body between them sixteen bytes per lane — and nothing outside the
// run is touched, read or written (the next element may be another plan's, in flight on another stream).
template <int ES>
__global__ __launch_bounds__(256) void k_erase(EraseArgs a) {
    typedef typename EraseElem<ES>::T T;
    constexpr int V = 16 / ES;                          // elements per 16-byte store
    const DevEraseJob job = a.jobs[blockIdx.x];
    const DevEraseRect rc = a.rects[job.rect];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T *slot = static_cast<T *>(a.dst) + rc.slot_off;
    const bool values = rc.kind == MJ_ERASE_VALUES;
    const T *vals = values ? static_cast<const T *>(a.values) + rc.src_off : nullptr;
    for (int r = job.run0 + wave; r < job.run0 + job.n_runs; r += 4) {
        const EraseRun run = erase_run(a.canvas, rc.x, rc.y, rc.w, rc.h, r);
        T *p = slot + run.first;
        // element e of the run: pixel e / group along it, component comp + e % group
        auto elem = [&](int px, int c) -> T {
            const int k = run.comp + c;                 // (selected, not indexed: the record stays in registers)
            return values ? vals[run.src + (int64_t)px * run.src_step + c * run.src_cstep] : (T)(k == 0 ? rc.bits[0] : k == 1 ? rc.bits[1] : rc.bits[2]);
        };
        const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
        if (addr % ES) {                                // (an array that is not aligned to its own elements: no vector body)
            for (int e = lane; e < run.len; e += 64) p[e] = elem(e / run.group, e % run.group);
            continue;
        }
        const int mis = (int)((addr & 15) / ES);
        int head = mis ? V - mis : 0;
        if (head > run.len) head = run.len;
        const int body = (run.len - head) / V, tail0 = head + body * V;
        if (lane < head) p[lane] = elem(lane / run.group, lane % run.group);
        for (int v = lane; v < body; v += 64) {
            const int e0 = head + v * V;
            int px = e0 / run.group, c = e0 - px * run.group;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < V; ++i) {
                w[i * ES / 4] |= (uint32_t)elem(px, c) << (8 * (i * ES % 4));
                if (++c == run.group) { c = 0; ++px; }
            }
            mj_eu32x4 q;
            q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
            *reinterpret_cast<mj_eu32x4 *>(p + e0) = q;
        }
        const int t = tail0 + lane;
        if (t < run.len) p[t] = elem(t / run.group, t % run.group);       // (fewer than V elements: one lane each)
    }
}

hipError_t launch_erase(hipStream_t stream, const EraseArgs &a, int esize) {
    if (a.n_jobs <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.n_jobs), block(256);
    if (esize == 1) hipLaunchKernelGGL(k_erase<1>, grid, block, 0, stream, a);
    else if (esize == 2) hipLaunchKernelGGL(k_erase<2>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_erase<4>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace mj

namespace {

uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// float32 -> float16, round to nearest even (overflow to infinity, gradual underflow)
uint16_t to_half(float f) {
    const uint32_t x = bits_of(f), sign = (x >> 16) & 0x8000u, m = x & 0x7FFFFFFFu;
    if (m > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);
    if (m >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);
    if (m < 0x38800000u) {
        // below 2^-14: adding 0.5 leaves the value in units of 2^-24 in the low mantissa bits, rounded by the addition itself
        float a;
        memcpy(&a, &m, 4);
        volatile float sum = a + 0.5f;
        return (uint16_t)(sign | (bits_of(sum) - 0x3F000000u));
    }
    const uint32_t r = m - 0x38000000u + 0xFFFu + ((m >> 13) & 1u);
    return (uint16_t)(sign | (r >> 13));
}

uint16_t to_bfloat(float f) {
    const uint32_t x = bits_of(f);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

// One record checked against the array it goes into and resolved (the message names the box); slots[output] (NULL: the output
// itself) is its slot.  false: `why` says what is wrong with it
bool resolve_rect(const mj_erase_rect &r, int k, int n_outputs, const int32_t *slots, const mj::EraseCanvas &cv, int dtype, bool have_values,
                  mj::DevEraseRect *out, char *why, size_t cap) {
    auto no = [&](const char *what) { snprintf(why, cap, "box %d (output %d, x %d, y %d, %d x %d): %s", k, r.output, r.x, r.y, r.width, r.height, what); return false; };
    if (r.output < 0 || r.output >= n_outputs) return no("no such output");
    if (r.width < 1 || r.height < 1) return no("a width or height below 1");
    if (r.x < 0 || r.y < 0 || (int64_t)r.x + r.width > cv.ow || (int64_t)r.y + r.height > cv.oh) return no("not inside the canvas");
    mj::DevEraseRect d{};
    d.slot_off = (int64_t)(slots ? slots[r.output] : r.output) * cv.ow * cv.oh * cv.C;
    d.x = r.x; d.y = r.y; d.w = r.width; d.h = r.height; d.kind = r.kind;
    if (r.kind == MJ_ERASE_VALUES) {
        if (!have_values) return no("a box of values without values");
        if (r.offset < 0) return no("a negative offset");
        d.src_off = r.offset;
    } else if (r.kind == MJ_ERASE_CONST) {
        for (int c = 0; c < cv.C; ++c) {
            const float v = r.value[c];
            if (!isfinite(v)) return no("a value that is not finite");
            if (dtype == MJ_DTYPE_U8) {
                if (v < 0.f || v > 255.f || v != floorf(v)) return no("a value that is not an integer 0..255 for a uint8 output");
                d.bits[c] = (uint32_t)(int)v;
            } else {
                d.bits[c] = dtype == MJ_DTYPE_F32 ? bits_of(v) : dtype == MJ_DTYPE_F16 ? to_half(v) : to_bfloat(v);
            }
        }
    } else {
        return no("a kind that is neither MJ_ERASE_CONST nor MJ_ERASE_VALUES");
    }
    *out = d;
    return true;
}

// the boxes sorted into launches: one where no two boxes of one output intersect, else one per box ordinal.  order: the boxes
// launch after launch; first[l] .. first[l + 1]: those of launch l
void erase_order(const std::vector<mj::DevEraseRect> &rects, std::vector<int32_t> &order, std::vector<int32_t> &first) {
    const int n = (int)rects.size();
    std::vector<int32_t> idx((size_t)n), ordinal((size_t)n, 0);
    for (int i = 0; i < n; ++i) idx[(size_t)i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return rects[(size_t)a].slot_off < rects[(size_t)b].slot_off; });
    bool meet = false;
    int deepest = 0;
    for (int i = 0; i < n;) {                           // (the boxes of one output: a run of idx, in the order they were listed)
        int j = i;
        while (j < n && rects[(size_t)idx[(size_t)j]].slot_off == rects[(size_t)idx[(size_t)i]].slot_off) ++j;
        for (int a = i; a < j; ++a) {
            ordinal[(size_t)idx[(size_t)a]] = a - i;
            const mj::DevEraseRect &p = rects[(size_t)idx[(size_t)a]];
            for (int b = i; b < a && !meet; ++b) {
                const mj::DevEraseRect &q = rects[(size_t)idx[(size_t)b]];
                meet = p.x < q.x + q.w && q.x < p.x + p.w && p.y < q.y + q.h && q.y < p.y + p.h;
            }
        }
        deepest = std::max(deepest, j - i);
        i = j;
    }
    order.clear(); first.clear();
    first.push_back(0);
    if (!meet) {
        for (int i = 0; i < n; ++i) order.push_back(i);
        first.push_back(n);
        return;
    }
    for (int o = 0; o < deepest; ++o) {
        for (int i = 0; i < n; ++i)
            if (ordinal[(size_t)i] == o) order.push_back(i);
        first.push_back((int32_t)order.size());
    }
}

template <typename T>
void host_erase_runs(T *array, const void *values, const mj::EraseCanvas &cv, const mj::DevEraseRect &rc) {
    T *slot = array + rc.slot_off;
    const T *vals = rc.kind == MJ_ERASE_VALUES ? static_cast<const T *>(values) + rc.src_off : nullptr;
    const int runs = mj::erase_run_count(cv, rc.w, rc.h);
    for (int r = 0; r < runs; ++r) {
        const mj::EraseRun run = mj::erase_run(cv, rc.x, rc.y, rc.w, rc.h, r);
        for (int e = 0; e < run.len; ++e) {
            const int px = e / run.group, c = e % run.group;
            slot[run.first + e] = vals ? vals[run.src + (int64_t)px * run.src_step + c * run.src_cstep] : (T)rc.bits[run.comp + c];
        }
    }
}

}  // namespace

// the erase launches of one execute, behind everything else it queued on s (api.hip: resize_launch)
int mj::erase_execute(mj_plan *p, hipStream_t s) {
    if (p->er_launches.empty()) return MJ_OK;
    mj::EraseArgs a{};
    a.dst = p->last_rgb; a.rects = p->d_er_rects; a.values = p->er_values;
    a.canvas = mj::EraseCanvas{p->rz.ow, p->rz.oh, p->er_C, p->layout};
    for (const auto &l : p->er_launches) {
        a.jobs = p->d_er_jobs + l[0]; a.n_jobs = l[1];
        MJ_HIP(p->ctx, mj::launch_erase(s, a, mj::erase_esize(p->er_dtype)));
    }
    return MJ_OK;
}

extern "C" {

int mj_plan_set_erase(mj_plan *p, int32_t n, const mj_erase_rect *rects, const void *values_device) {
    if (!p) return MJ_ERR_INVALID;
    mj_context *ctx = p->ctx;
    const char *fn = "mj_plan_set_erase";
    if (!p->resized || p->orient_only) return fail(ctx, MJ_ERR_INVALID, "%s: erase needs a size (a plan with out_width / out_height)", fn);
    if (n < 0) return fail(ctx, MJ_ERR_INVALID, "%s: n = %d", fn, n);
    if (n > 0 && !rects) return fail(ctx, MJ_ERR_INVALID, "%s: rects is NULL with n = %d", fn, n);
    const mj::EraseCanvas cv{p->rz.ow, p->rz.oh, p->er_C, p->layout};
    std::vector<mj::DevEraseRect> dev((size_t)n);
    char why[256];
    for (int k = 0; k < n; ++k)
        if (!resolve_rect(rects[k], k, (int)p->h_slot.size(), p->h_slot.data(), cv, p->er_dtype, values_device != nullptr, &dev[(size_t)k], why, sizeof(why)))
            return fail(ctx, MJ_ERR_INVALID, "%s: %s", fn, why);
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    // the records an execute in flight reads, and the graph that holds their addresses, go: wait for that execute first
    if (p->done_valid) MJ_HIP(ctx, hipEventSynchronize(p->done));
    if (p->graph_exec) { (void)hipGraphExecDestroy(p->graph_exec); p->graph_exec = nullptr; }
    p->graph_stream = nullptr; p->prev_stream = nullptr; p->last_was_graph = false;
    p->er_launches.clear(); p->er_values = nullptr; p->er_bytes = 0;
    if (n == 0) return MJ_OK;
    std::vector<int32_t> order, first;
    erase_order(dev, order, first);
    std::vector<mj::DevEraseJob> jobs;
    std::vector<std::array<int32_t, 2>> launches;
    for (size_t l = 0; l + 1 < first.size(); ++l) {
        const int32_t at = (int32_t)jobs.size();
        mj::erase_jobs(cv, dev.data(), order.data() + first[l], first[l + 1] - first[l], jobs);
        launches.push_back({at, (int32_t)jobs.size() - at});
    }
    if (int rc = upload(p, &p->d_er_rects, dev.data(), dev.size())) return rc;
    if (int rc = upload(p, &p->d_er_jobs, jobs.data(), jobs.size())) return rc;
    for (const auto &d : dev) p->er_bytes += (int64_t)d.w * d.h * cv.C * mj::erase_esize(p->er_dtype);
    p->er_values = values_device;
    p->er_launches = launches;
    return MJ_OK;
}

int mj_plan_time_erase(mj_plan *p, int iters, float *ms_out, int64_t *bytes_written) {
    if (!p || iters <= 0 || !ms_out) return MJ_ERR_INVALID;
    mj_context *ctx = p->ctx;
    if (p->er_launches.empty()) return fail(ctx, MJ_ERR_INVALID, "mj_plan_time_erase: no erase set on this plan (mj_plan_set_erase)");
    if (!p->last_rgb) return fail(ctx, MJ_ERR_INVALID, "mj_plan_time_erase: nothing executed yet");
    hipStream_t s = ctx->stream;
    if (p->done_valid) MJ_HIP(ctx, hipEventSynchronize(p->done));
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    MJ_HIP(ctx, hipEventCreate(&ev.a));
    MJ_HIP(ctx, hipEventCreate(&ev.b));
    if (int rc = mj::erase_execute(p, s)) return rc;            // (warm)
    MJ_HIP(ctx, hipEventRecord(ev.a, s));
    for (int i = 0; i < iters; ++i)
        if (int rc = mj::erase_execute(p, s)) return rc;
    MJ_HIP(ctx, hipEventRecord(ev.b, s));
    MJ_HIP(ctx, hipEventSynchronize(ev.b));
    float ms = 0.f;
    MJ_HIP(ctx, hipEventElapsedTime(&ms, ev.a, ev.b));
    *ms_out = ms / iters;
    if (bytes_written) *bytes_written = p->er_bytes;
    MJ_HIP(ctx, hipEventRecord(p->done, s));
    p->done_valid = true;
    return MJ_OK;
}

int mj_host_erase(void *array, int32_t layout, int32_t dtype, int32_t ncomp, int32_t width, int32_t height, int32_t n_slots, int32_t n,
                  const mj_erase_rect *rects, const void *values) {
    const char *fn = "mj_host_erase";
    if (!array || n < 0 || (n > 0 && !rects)) return fail(nullptr, MJ_ERR_INVALID, "%s: NULL argument or n < 0", fn);
    if (layout < 0 || layout > 3 || !mj::erase_esize(dtype) || (ncomp != 1 && ncomp != 3) || width < 1 || height < 1 || width > 65535 ||
        height > 65535 || n_slots < 1)
        return fail(nullptr, MJ_ERR_INVALID, "%s: layout %d, dtype %d, %d components, %d x %d, %d slots", fn, layout, dtype, ncomp, width, height, n_slots);
    const mj::EraseCanvas cv{width, height, ncomp, layout};
    std::vector<mj::DevEraseRect> dev((size_t)n);
    char why[256];
    for (int k = 0; k < n; ++k)
        if (!resolve_rect(rects[k], k, n_slots, nullptr, cv, dtype, values != nullptr, &dev[(size_t)k], why, sizeof(why)))
            return fail(nullptr, MJ_ERR_INVALID, "%s: %s", fn, why);
    // in the launches' order, which keeps every output's boxes in the order they were listed
    std::vector<int32_t> order, first;
    erase_order(dev, order, first);
    for (int32_t k : order) {
        const mj::DevEraseRect &rc = dev[(size_t)k];
        switch (mj::erase_esize(dtype)) {
            case 1: host_erase_runs(static_cast<uint8_t *>(array), values, cv, rc); break;
            case 2: host_erase_runs(static_cast<uint16_t *>(array), values, cv, rc); break;
            default: host_erase_runs(static_cast<uint32_t *>(array), values, cv, rc); break;
        }
    }
    return MJ_OK;
}

}  // extern "C"
