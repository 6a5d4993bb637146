// Compose (mj_compose; tools/compose_model.py): several finished outputs of a CALL pasted onto one canvas — mosaics, grids, a crop
// of one sample in another — as the last step behind erase.  A canvas's tiles may be any plans' outputs, so, like mix (mix.hip),
// this launch belongs to no plan: it reads one array of slots and writes another of another size.  The kernel, its launch, the
// call, its timing twin and the host twins.  Which rectangle of a canvas comes from where is resolved on the host
// (compose_addr.h): the kernel copies disjoint rectangles and never sees an overlap.
#include "plan.h"
#include "compose_addr.h"

namespace mj {

typedef unsigned int mj_cu32x4 __attribute__((ext_vector_type(4)));
template <int ES> struct ComposeElem;
template <> struct ComposeElem<1> { typedef uint8_t T; };
template <> struct ComposeElem<2> { typedef uint16_t T; };
template <> struct ComposeElem<4> { typedef uint32_t T; };

// the 16 bytes of a fill vector whose first element has component `phase` (three interleaved components; else b0 == b1 == b2)
template <int ES>
__device__ __forceinline__ mj_cu32x4 fill_vector(int phase, uint32_t b0, uint32_t b1, uint32_t b2) {
    constexpr int V = 16 / ES, PER = 4 / ES;
    const uint32_t b[3] = {b0, b1, b2};
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < V; ++i) w[i / PER] |= b[(phase + i) % 3] << (8 * ES * (i % PER));
    mj_cu32x4 o;
    o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    return o;
}

// A streaming kernel: one workgroup per job (compose_addr.h: lines of one rectangle, about kComposeJobBytes of them), the stride
// loop only for what a grid cannot hold.  P = 1 << shift lanes share a line and 256 / P lines are under way at a time, so the
// line is the loop variable and its two addresses are one multiply-add each: no division anywhere but the fill's phase mod 3.
// Within a line the lanes take the 16-byte vectors of the DESTINATION's aligned body, one global_store_dwordx4 each; the source
// bytes are loaded from wherever they land — an address only known to be element-aligned, which the target's global loads take
// (one global_load_dwordx4, as k_mix loads its partner) —; the elements in front of the first 16-byte boundary and behind the last
// go one lane each.  kComposeUnroll lines per lane are loaded before any is stored.  Every destination element is written exactly
// once, the destination is never read, and no store reaches over the rectangle's edge: the neighbour is another workgroup's.
template <int ES>
__global__ __launch_bounds__(256) void k_compose(ComposeArgs a) {
    typedef typename ComposeElem<ES>::T T;
    constexpr int V = 16 / ES, U = kComposeUnroll;
    constexpr uint32_t EMASK = ES == 4 ? 0xFFFFFFFFu : (1u << (8 * (ES & 3))) - 1u;
    const int tid = threadIdx.x;
    for (int jb = blockIdx.x; jb < a.n_jobs; jb += gridDim.x) {
        const DevComposeJob job = a.jobs[jb];
        const int P = 1 << job.shift, LP = 256 >> job.shift;
        const int j = tid & (P - 1), first = tid >> job.shift;
        const int len = job.len, nlines = job.nlines;
        T *const d0 = static_cast<T *>(a.dst) + job.dst;
        // elements in front of the first 16-byte boundary of a line that starts at p (p is element-aligned: mj_compose checks)
        auto head_of = [&](const T *p) {
            const int h = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / ES);
            return h < len ? h : len;
        };
        if (job.src < 0) {
            const uint32_t own = job.comp == 0 ? a.fill[0] : job.comp == 1 ? a.fill[1] : a.fill[2];       // (a plane's; no indexed kernel argument)
            const uint32_t b0 = (a.C3 ? a.fill[0] : own) & EMASK, b1 = (a.C3 ? a.fill[1] : own) & EMASK, b2 = (a.C3 ? a.fill[2] : own) & EMASK;
            const mj_cu32x4 pat0 = fill_vector<ES>(0, b0, b1, b2), pat1 = fill_vector<ES>(1, b0, b1, b2), pat2 = fill_vector<ES>(2, b0, b1, b2);
            auto one = [&](T *d, int e) { const unsigned ph = (unsigned)e % 3u; d[e] = (T)(ph == 0 ? b0 : ph == 1 ? b1 : b2); };
            for (int l = first; l < nlines; l += LP) {
                T *d = d0 + (int64_t)l * a.dst_stride;
                const int h = head_of(d), nb = (len - h) / V;
                for (int e = j; e < h; e += P) one(d, e);
                for (int e = h + nb * V + j; e < len; e += P) one(d, e);
                for (int v = j; v < nb; v += P) {
                    const unsigned ph = (unsigned)(h + v * V) % 3u;
                    *reinterpret_cast<mj_cu32x4 *>(d + h + v * V) = ph == 0 ? pat0 : ph == 1 ? pat1 : pat2;
                }
            }
            continue;
        }
        const T *const s0 = static_cast<const T *>(a.src) + job.src;
        for (int l0 = first; l0 < nlines; l0 += LP * U) {
            int64_t doff[U], soff[U];                   // (offsets, not pointers: the accesses stay global ones)
            int nb[U], most = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int l = l0 + u * LP;
                nb[u] = 0; doff[u] = 0; soff[u] = 0;
                if (l < nlines) {
                    T *dl = d0 + (int64_t)l * a.dst_stride;
                    const T *sl = s0 + (int64_t)l * a.src_stride;
                    const int h = head_of(dl);
                    nb[u] = (len - h) / V;
                    for (int e = j; e < h; e += P) dl[e] = sl[e];
                    for (int e = h + nb[u] * V + j; e < len; e += P) dl[e] = sl[e];
                    doff[u] = (int64_t)l * a.dst_stride + h; soff[u] = (int64_t)l * a.src_stride + h;       // (the aligned body)
                }
                most = nb[u] > most ? nb[u] : most;
            }
            for (int v = j; v < most; v += P) {
                mj_cu32x4 r[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (v < nb[u]) __builtin_memcpy(&r[u], s0 + soff[u] + (int64_t)v * V, 16);
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (v < nb[u]) *reinterpret_cast<mj_cu32x4 *>(d0 + doff[u] + (int64_t)v * V) = r[u];
            }
        }
    }
}

hipError_t launch_compose(hipStream_t stream, const ComposeArgs &a, int esize) {
    if (a.n_jobs < 1) return hipSuccess;
    // One workgroup per job, as launch_mix has one per piece; not measured against a capped grid that strides
    // (tools/compose_probe.py measures the launch beside k_copy16 over the same bytes).
    constexpr int cap = 1 << 22;
    const dim3 grid((unsigned)(a.n_jobs < cap ? a.n_jobs : cap)), block(256);
    if (esize == 1) hipLaunchKernelGGL(k_compose<1>, grid, block, 0, stream, a);
    else if (esize == 2) hipLaunchKernelGGL(k_compose<2>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_compose<4>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace mj

static_assert(sizeof(mj_compose_tile) == sizeof(mj::ComposeTile) && sizeof(mj_compose_rect) == sizeof(mj::ComposeRect), "compose_addr.h restates mijpeg.h's records");

namespace {

// the description of the canvases and the tiles checked; false: `why` says what is wrong with it (naming the tile)
bool check_geometry(int layout, int ncomp, int sw, int sh, int n_sources, int dw, int dh, int n_outputs, int n_tiles, const mj_compose_tile *tiles,
                    char *why, size_t cap) {
    if (layout < 0 || layout > 3 || (ncomp != 1 && ncomp != 3) || sw < 1 || sh < 1 || sw > 65535 || sh > 65535 || dw < 1 || dh < 1 || dw > 65535 ||
        dh > 65535 || n_sources < 1 || n_outputs < 1 || n_tiles < 0) {
        snprintf(why, cap, "layout %d, %d components, %d sources of %d x %d, %d outputs of %d x %d, %d tiles", layout, ncomp, n_sources, sw, sh, n_outputs, dw, dh, n_tiles);
        return false;
    }
    if (n_tiles && !tiles) { snprintf(why, cap, "NULL argument"); return false; }
    std::vector<int> count((size_t)n_outputs, 0);
    for (int t = 0; t < n_tiles; ++t) {
        const mj_compose_tile &q = tiles[t];
        auto no = [&](const char *what) {
            snprintf(why, cap, "tile %d (output %d, source %d, window %d, %d, %d x %d, to %d, %d): %s", t, q.output, q.source, q.sx, q.sy, q.width, q.height, q.dx, q.dy, what);
            return false;
        };
        if (q.output < 0 || q.output >= n_outputs) return no("no such output");
        if (q.source < 0 || q.source >= n_sources) return no("no such source");
        if (q.width < 1 || q.height < 1) return no("a width or height below 1");
        if (q.sx < 0 || q.sy < 0 || (int64_t)q.sx + q.width > sw || (int64_t)q.sy + q.height > sh) return no("the window is not inside the source canvas");
        if (q.dx <= -mj::kComposeMaxOffset || q.dx >= mj::kComposeMaxOffset || q.dy <= -mj::kComposeMaxOffset || q.dy >= mj::kComposeMaxOffset)
            return no("an offset of 2^20 or more");
        if (++count[(size_t)q.output] > mj::kComposeMaxTiles) return no("more than 64 tiles in one output");
    }
    return true;
}

bool check_arrays(const void *src, const void *dst, int dtype, int ncomp, int sw, int sh, int n_sources, int dw, int dh, int n_outputs, const uint32_t *fill,
                  char *why, size_t cap) {
    if (!src || !dst || !fill) { snprintf(why, cap, "NULL argument"); return false; }
    const int es = mj::erase_esize(dtype);
    if (!es) { snprintf(why, cap, "dtype %d", dtype); return false; }
    const uint64_t sslot = (uint64_t)sw * sh * ncomp * es, dslot = (uint64_t)dw * dh * ncomp * es;      // (below 2^36)
    if ((uint64_t)n_sources > ((uint64_t)1 << 62) / sslot || (uint64_t)n_outputs > ((uint64_t)1 << 62) / dslot) {
        snprintf(why, cap, "%d sources of %llu bytes, %d outputs of %llu bytes: more than an address holds", n_sources, (unsigned long long)sslot, n_outputs,
                 (unsigned long long)dslot);
        return false;
    }
    const uint64_t sbytes = (uint64_t)n_sources * sslot, dbytes = (uint64_t)n_outputs * dslot;
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (s % es || d % es) { snprintf(why, cap, "src or dst is not aligned to its %d-byte elements", es); return false; }
    if (s < d + dbytes && d < s + sbytes) { snprintf(why, cap, "src and dst overlap (%llu and %llu bytes)", (unsigned long long)sbytes, (unsigned long long)dbytes); return false; }
    return true;
}

// every output's rectangles, outputs in order (the tiles need not be grouped by output; within one they keep their order)
void resolve(const mj::ComposeGeom &g, int n_outputs, int n_tiles, const mj_compose_tile *tiles, std::vector<mj::ComposeRect> &rects) {
    std::vector<std::vector<mj::ComposeTile>> per((size_t)n_outputs);
    for (int t = 0; t < n_tiles; ++t) {
        const mj_compose_tile &q = tiles[t];
        per[(size_t)q.output].push_back(mj::ComposeTile{q.output, q.source, q.sx, q.sy, q.width, q.height, q.dx, q.dy});
    }
    for (int m = 0; m < n_outputs; ++m) mj::compose_resolve_output(g, m, per[(size_t)m].data(), (int)per[(size_t)m].size(), rects);
}

// checked and resolved: the jobs of a launch (or of the host twin's walk) and its arguments but for the pointers
int compose_prepare(mj_context *ctx, const char *fn, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t sw, int32_t sh,
                    int32_t n_sources, int32_t dw, int32_t dh, int32_t n_outputs, const uint32_t *fill, int32_t n_tiles, const mj_compose_tile *tiles,
                    std::vector<mj::DevComposeJob> &jobs, mj::ComposeArgs *a) {
    char why[320];
    if (!check_geometry(layout, ncomp, sw, sh, n_sources, dw, dh, n_outputs, n_tiles, tiles, why, sizeof(why)) ||
        !check_arrays(src, dst, dtype, ncomp, sw, sh, n_sources, dw, dh, n_outputs, fill, why, sizeof(why)))
        return fail(ctx, MJ_ERR_INVALID, "%s: %s", fn, why);
    const mj::ComposeGeom g{sw, sh, dw, dh, ncomp, layout};
    std::vector<mj::ComposeRect> rects;
    resolve(g, n_outputs, n_tiles, tiles, rects);
    for (const mj::ComposeRect &r : rects) mj::compose_jobs(g, mj::erase_esize(dtype), r, jobs);
    if (jobs.size() > (size_t)0x7FFFFFFF) return fail(ctx, MJ_ERR_INVALID, "%s: %zu jobs: more than a launch holds", fn, jobs.size());
    mj::compose_args(g, fill, a);
    a->src = src; a->dst = dst; a->jobs = nullptr; a->n_jobs = (int32_t)jobs.size();
    return MJ_OK;
}

// the jobs into the context's device buffer, behind the previous compose launch (which reads it), ahead of this one on `s`
int stage_jobs(mj_context *ctx, hipStream_t s, const std::vector<mj::DevComposeJob> &jobs) {
    const size_t bytes = jobs.size() * sizeof(mj::DevComposeJob);
    if (ctx->compose_flying) { MJ_HIP(ctx, hipEventSynchronize(ctx->compose_done)); ctx->compose_flying = false; }
    if (!ctx->compose_done) MJ_HIP(ctx, hipEventCreateWithFlags(&ctx->compose_done, hipEventDisableTiming));
    if (bytes > ctx->compose_cap) {
        if (ctx->h_compose) { (void)hipHostFree(ctx->h_compose); ctx->h_compose = nullptr; }
        if (ctx->d_compose) { (void)hipFree(ctx->d_compose); ctx->d_compose = nullptr; }
        ctx->compose_cap = 0;
        const size_t cap = bytes + bytes / 2 + 4096;
        MJ_HIP(ctx, hipHostMalloc(&ctx->h_compose, cap, hipHostMallocDefault));
        MJ_HIP(ctx, hipMalloc(&ctx->d_compose, cap));
        ctx->compose_cap = cap;
    }
    memcpy(ctx->h_compose, jobs.data(), bytes);
    MJ_HIP(ctx, hipMemcpyAsync(ctx->d_compose, ctx->h_compose, bytes, hipMemcpyHostToDevice, s));
    return MJ_OK;
}

template <typename T>
void host_compose(const T *src, T *dst, const mj::ComposeArgs &a, const std::vector<mj::DevComposeJob> &jobs) {
    for (const mj::DevComposeJob &job : jobs)
        for (int l = 0; l < job.nlines; ++l) {
            T *d = dst + job.dst + (int64_t)l * a.dst_stride;
            if (job.src < 0) {
                for (int e = 0; e < job.len; ++e) d[e] = (T)a.fill[a.C3 ? e % 3 : job.comp];
                continue;
            }
            const T *s = src + job.src + (int64_t)l * a.src_stride;
            for (int e = 0; e < job.len; ++e) d[e] = s[e];
        }
}

}  // namespace

extern "C" {

int mj_compose(mj_context *ctx, void *stream, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width,
               int32_t src_height, int32_t n_sources, int32_t dst_width, int32_t dst_height, int32_t n_outputs, const uint32_t fill_bits[3],
               int32_t n_tiles, const mj_compose_tile *tiles) {
    if (!ctx) return MJ_ERR_INVALID;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    mj::ComposeArgs a{};
    std::vector<mj::DevComposeJob> jobs;
    if (int rc = compose_prepare(ctx, "mj_compose", src, dst, layout, dtype, ncomp, src_width, src_height, n_sources, dst_width, dst_height, n_outputs,
                                 fill_bits, n_tiles, tiles, jobs, &a))
        return rc;
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = stage_jobs(ctx, s, jobs)) return rc;
    a.jobs = static_cast<const mj::DevComposeJob *>(ctx->d_compose);
    // (the event goes behind the staging copy whether or not the launch went out, as in mj_mix)
    const hipError_t launched = mj::launch_compose(s, a, mj::erase_esize(dtype));
    const hipError_t recorded = hipEventRecord(ctx->compose_done, s);
    if (recorded == hipSuccess) ctx->compose_flying = true;
    else (void)hipStreamSynchronize(s);
    MJ_HIP(ctx, launched);
    MJ_HIP(ctx, recorded);
    return MJ_OK;
}

int mj_compose_time(mj_context *ctx, int iters, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width,
                    int32_t src_height, int32_t n_sources, int32_t dst_width, int32_t dst_height, int32_t n_outputs, const uint32_t fill_bits[3],
                    int32_t n_tiles, const mj_compose_tile *tiles, float *ms_out) {
    if (!ctx || iters <= 0 || !ms_out) return MJ_ERR_INVALID;
    hipStream_t s = ctx->stream;
    mj::ComposeArgs a{};
    std::vector<mj::DevComposeJob> jobs;
    if (int rc = compose_prepare(ctx, "mj_compose_time", src, dst, layout, dtype, ncomp, src_width, src_height, n_sources, dst_width, dst_height, n_outputs,
                                 fill_bits, n_tiles, tiles, jobs, &a))
        return rc;
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = stage_jobs(ctx, s, jobs)) return rc;
    a.jobs = static_cast<const mj::DevComposeJob *>(ctx->d_compose);
    // (the staged jobs are read until the last launch ends: every way out of here leaves the stream drained, so compose_flying stays false)
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{s};
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    const int es = mj::erase_esize(dtype);
    MJ_HIP(ctx, hipEventCreate(&ev.a));
    MJ_HIP(ctx, hipEventCreate(&ev.b));
    MJ_HIP(ctx, mj::launch_compose(s, a, es));          // (warm)
    MJ_HIP(ctx, hipEventRecord(ev.a, s));
    for (int i = 0; i < iters; ++i) MJ_HIP(ctx, mj::launch_compose(s, a, es));
    MJ_HIP(ctx, hipEventRecord(ev.b, s));
    MJ_HIP(ctx, hipEventSynchronize(ev.b));
    float ms = 0.f;
    MJ_HIP(ctx, hipEventElapsedTime(&ms, ev.a, ev.b));
    *ms_out = ms / iters;
    return MJ_OK;
}

int mj_host_compose(const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height, int32_t n_sources,
                    int32_t dst_width, int32_t dst_height, int32_t n_outputs, const uint32_t fill_bits[3], int32_t n_tiles, const mj_compose_tile *tiles) {
    mj::ComposeArgs a{};
    std::vector<mj::DevComposeJob> jobs;
    if (int rc = compose_prepare(nullptr, "mj_host_compose", src, dst, layout, dtype, ncomp, src_width, src_height, n_sources, dst_width, dst_height, n_outputs,
                                 fill_bits, n_tiles, tiles, jobs, &a))
        return rc;
    switch (mj::erase_esize(dtype)) {
        case 1: host_compose(static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), a, jobs); break;
        case 2: host_compose(static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst), a, jobs); break;
        default: host_compose(static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), a, jobs); break;
    }
    return MJ_OK;
}

int mj_host_compose_resolve(int32_t layout, int32_t ncomp, int32_t src_width, int32_t src_height, int32_t n_sources, int32_t dst_width, int32_t dst_height,
                            int32_t n_outputs, int32_t n_tiles, const mj_compose_tile *tiles, mj_compose_rect *rects, int32_t cap, int32_t *n_rects) {
    const char *fn = "mj_host_compose_resolve";
    char why[320];
    if (!n_rects || cap < 0) return fail(nullptr, MJ_ERR_INVALID, "%s: NULL argument", fn);
    if (!check_geometry(layout, ncomp, src_width, src_height, n_sources, dst_width, dst_height, n_outputs, n_tiles, tiles, why, sizeof(why)))
        return fail(nullptr, MJ_ERR_INVALID, "%s: %s", fn, why);
    if (!rects) {                                       // the capacity that always suffices
        std::vector<int64_t> count((size_t)n_outputs, 0);
        for (int t = 0; t < n_tiles; ++t) ++count[(size_t)tiles[t].output];
        int64_t bound = 0;
        for (int64_t c : count) bound += mj::compose_rect_bound(c);
        *n_rects = (int32_t)std::min<int64_t>(bound, 0x7FFFFFFF);
        return MJ_OK;
    }
    std::vector<mj::ComposeRect> found;
    resolve(mj::ComposeGeom{src_width, src_height, dst_width, dst_height, ncomp, layout}, n_outputs, n_tiles, tiles, found);
    *n_rects = (int32_t)std::min<size_t>(found.size(), 0x7FFFFFFF);
    if (found.size() > (size_t)cap) return fail(nullptr, MJ_ERR_INVALID, "%s: %zu rectangles for a capacity of %d", fn, found.size(), cap);
    for (size_t i = 0; i < found.size(); ++i) {
        const mj::ComposeRect &r = found[i];
        rects[i] = mj_compose_rect{r.output, r.x, r.y, r.w, r.h, r.source, r.sx, r.sy};
    }
    return MJ_OK;
}

}  // extern "C"
