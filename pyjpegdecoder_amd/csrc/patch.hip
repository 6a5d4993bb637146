// Patchify (mj_patchify; tools/patch_model.py): the finished outputs of a CALL cut into P x P patches and packed as the token rows
// of a native-resolution vision encoder — Qwen2-VL's (C, t, P, P) tokens in merge blocks, NaFlex's (P, P, C) tokens —, the last
// step behind erase, mix and compose.  Like mix and compose a launch of the call, not of a plan: it reads one array of slots and
// writes a matrix of another shape.  The kernel, its launch, the call, its timing twin and the host twins.  Which element lands
// where is patch_addr.h's.
#include "plan.h"
#include "patch_addr.h"

namespace mj {

typedef unsigned int mj_pu32x4 __attribute__((ext_vector_type(4)));
template <int ES> struct PatchElem;
template <> struct PatchElem<1> { typedef uint8_t T; };
template <> struct PatchElem<2> { typedef uint16_t T; };
template <> struct PatchElem<4> { typedef uint32_t T; };

constexpr int kPatchUnroll = 4;                     // vectors a lane has loaded before it scatters any

// A real permutation, so through the LDS: one workgroup per job (patch_addr.h: a run of merge blocks of one band, whose tokens
// are ONE contiguous range of the destination), the stride loop only for what a grid cannot hold.
//
// Phase 1: the job's source rectangle is read along the layout's contiguous axis — rows, or columns in the x-major layouts, one
// component plane at a time in the planar ones — in 16-byte vectors from wherever the bytes land: a line is only known to be
// element-aligned, which the target's global loads take (as k_compose and k_mix load).  A line gets 1 << shift lanes, the next
// power of two above its vectors, so a lane's line and vector are a shift and a mask.  kPatchUnroll vectors are loaded before
// any is scattered.  The elements of a vector go to the LDS image of the job's range in OUTPUT order, one ds_write each (t of
// them under repeat): the first element's place takes four multiplications by host-supplied reciprocals (patch_div), the
// others follow by counters that step and wrap.  No division instruction anywhere.
//
// Phase 2, behind the barrier: the image is streamed out, one global_store_dwordx4 per lane over the destination's 16-byte-aligned
// body, lone element stores in front of it and behind.  The image starts at the destination's address mod 16 in the LDS, so every
// 16-byte LDS read is naturally aligned (an unaligned ds_read_b128 is replayed).  Every destination element is written exactly
// once, the destination is never read, and no store reaches over the job's range: the neighbour is another workgroup's.  Fill
// jobs (the pad rows of the padded form) store zero vectors the same way and never touch the LDS.
//
// Dynamic LDS only: a static array beside it would shift its base off 16 bytes.
template <int ES>
__global__ __launch_bounds__(256) void k_patchify(PatchArgs a) {
    typedef typename PatchElem<ES>::T T;
    constexpr int V = 16 / ES, PER = 4 / ES, U = kPatchUnroll;
    constexpr uint32_t EMASK = ES == 4 ? 0xFFFFFFFFu : (1u << (8 * (ES & 3))) - 1u;
    extern __shared__ __attribute__((aligned(16))) unsigned char patch_lds[];
    const int tid = threadIdx.x;
    for (int jb = blockIdx.x; jb < a.n_jobs; jb += gridDim.x) {
        const DevPatchJob job = a.jobs[jb];
        T *const d0 = static_cast<T *>(a.dst) + job.dst;
        unsigned char *const db = reinterpret_cast<unsigned char *>(d0);
        const int off = (int)(reinterpret_cast<uintptr_t>(d0) & 15u);       // (a multiple of ES: mj_patchify checks dst)
        const bool fill = job.src < 0;
        const int nb = (fill ? job.count : job.count * a.m * a.m * a.D) * ES;   // bytes of the job's range, 65536 at the most
        int head = (16 - off) & 15;
        if (head > nb) head = nb;
        const int nvec = (nb - head) >> 4, tail0 = head + (nvec << 4);
        if (fill) {
            const mj_pu32x4 zero = {0u, 0u, 0u, 0u};
            for (int e = tid; e < head / ES; e += 256) d0[e] = (T)0;
            for (int v = tid; v < nvec; v += 256) *reinterpret_cast<mj_pu32x4 *>(db + head + 16 * v) = zero;
            for (int e = tail0 / ES + tid; e < nb / ES; e += 256) d0[e] = (T)0;
            continue;
        }
        // ---- phase 1: source lines -> the image, in output order
        T *const img = reinterpret_cast<T *>(patch_lds + off);
        const T *const s0 = static_cast<const T *>(a.src) + job.src;
        const int group = a.planar ? 1 : a.C;
        const int along = a.rows ? job.count * a.mP : a.mP, across = a.rows ? a.mP : job.count * a.mP;
        const int len = along * group, nlines = a.planar ? across * a.C : across;
        const int vpl = (len + V - 1) / V;
        const int shift = vpl > 1 ? 32 - __clz(vpl - 1) : 0;
        const int total = nlines << shift, mask = (1 << shift) - 1;
        const int PP = a.P * a.P, mm = a.m * a.m;
        for (int base = tid; base < total; base += 256 * U) {
            mj_pu32x4 r[U];
            int cnt[U], e0[U], line[U], plane[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = base + u * 256;
                cnt[u] = 0; e0[u] = 0; line[u] = 0; plane[u] = 0;
                r[u] = mj_pu32x4{0u, 0u, 0u, 0u};
                const int l = s >> shift, vi = s & mask;
                if (s < total && vi < vpl) {
                    int c = 0, v = l;
                    if (a.planar) { c = (l >= across) + (l >= 2 * across); v = l - c * across; }
                    e0[u] = vi * V; line[u] = v; plane[u] = c;
                    cnt[u] = len - e0[u] < V ? len - e0[u] : V;
                    const T *p = s0 + (int64_t)c * a.s_c + (int64_t)v * a.s_line + e0[u];
                    if (cnt[u] == V) {
                        __builtin_memcpy(&r[u], p, 16);
                    } else {                                // (the line's last elements: nothing is read beyond them)
                        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int q = 0; q < V; ++q)
                            if (q < cnt[u]) w[q / PER] |= (uint32_t)p[q] << (8 * ES * (q % PER) & 31);
                        r[u] = mj_pu32x4{w[0], w[1], w[2], w[3]};
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (cnt[u]) {
                    uint32_t px = (uint32_t)e0[u], c = (uint32_t)plane[u];
                    if (group == 3) { px = (uint32_t)e0[u] / 3u; c = (uint32_t)e0[u] - 3u * px; }
                    const uint32_t qa = patch_div(px, a.mulP), ablk = patch_div(qa, a.mulm);
                    const uint32_t qv = patch_div((uint32_t)line[u], a.mulP), vblk = patch_div(qv, a.mulm);
                    int ai = (int)(px - qa * a.P), ag = (int)(qa - ablk * a.m);
                    const int vi = (int)((uint32_t)line[u] - qv * a.P), vg = (int)(qv - vblk * a.m);
                    const int tok = (int)(ablk + vblk) * mm + ag * a.tok_step + vg * a.tok_across;
                    int pos = tok * a.D + vi * a.xs + (int)c * a.cs + ai * a.as;
                    const uint32_t w[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
#pragma unroll
                    for (int q = 0; q < V; ++q) {
                        if (q < cnt[u]) {
                            const T el = (T)((w[q / PER] >> (8 * ES * (q % PER) & 31)) & EMASK);
                            for (int rr = 0; rr < a.t; ++rr) img[pos + rr * PP] = el;
                            bool pixel = true;              // (the next element is the next pixel's)
                            if (group == 3) {
                                pos += a.cs;
                                if (++c < 3u) pixel = false;
                                else { c = 0u; pos -= 3 * a.cs; }
                            }
                            if (pixel) {
                                pos += a.as;
                                if (++ai == a.P) {
                                    ai = 0; pos += a.tok_step * a.D - a.P * a.as;
                                    if (++ag == a.m) { ag = 0; pos += a.tok_wrap * a.D; }
                                }
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- phase 2: the image -> the destination
        for (int e = tid; e < head / ES; e += 256) d0[e] = img[e];
        for (int v = tid; v < nvec; v += 256)
            *reinterpret_cast<mj_pu32x4 *>(db + head + 16 * v) = *reinterpret_cast<const mj_pu32x4 *>(patch_lds + off + head + 16 * v);
        for (int e = tail0 / ES + tid; e < nb / ES; e += 256) d0[e] = img[e];
        __syncthreads();                                // (the stride loop's next job rewrites the image)
    }
}

hipError_t launch_patchify(hipStream_t stream, const PatchArgs &a, int esize, size_t lds) {
    if (a.n_jobs < 1) return hipSuccess;
    // a merge block may be all of 64 KiB, and the image's slack goes on top
    static OncePerDevice attr_once;
    attr_once.run([&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_patchify<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kPatchBlockBytes + kPatchLdsSlack);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_patchify<2>), hipFuncAttributeMaxDynamicSharedMemorySize, kPatchBlockBytes + kPatchLdsSlack);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_patchify<4>), hipFuncAttributeMaxDynamicSharedMemorySize, kPatchBlockBytes + kPatchLdsSlack);
    });
    constexpr int cap = 1 << 22;
    const dim3 grid((unsigned)(a.n_jobs < cap ? a.n_jobs : cap)), block(256);
    if (esize == 1) hipLaunchKernelGGL(k_patchify<1>, grid, block, lds, stream, a);
    else if (esize == 2) hipLaunchKernelGGL(k_patchify<2>, grid, block, lds, stream, a);
    else hipLaunchKernelGGL(k_patchify<4>, grid, block, lds, stream, a);
    return hipGetLastError();
}

}  // namespace mj

static_assert(sizeof(mj_patch_window) == sizeof(mj::PatchWindow), "patch_addr.h restates mijpeg.h's record");

namespace {

// the description of the sources, the patches and the windows checked; false: `why` says what is wrong with it (naming the source)
bool check_geometry(int layout, int dtype, int ncomp, int sw, int sh, int n_sources, int P, int m, int t, int order, int length, const mj_patch_window *windows,
                    char *why, size_t cap) {
    const int es = mj::erase_esize(dtype);
    if (layout < 0 || layout > 3 || (ncomp != 1 && ncomp != 3) || sw < 1 || sh < 1 || sw > 65535 || sh > 65535 || n_sources < 1) {
        snprintf(why, cap, "layout %d, %d components, %d sources of %d x %d", layout, ncomp, n_sources, sw, sh);
        return false;
    }
    if (!es) { snprintf(why, cap, "dtype %d", dtype); return false; }
    if (P < 1 || P > mj::kPatchMaxPatch) { snprintf(why, cap, "patch %d is not 1..%d", P, mj::kPatchMaxPatch); return false; }
    if (m < 1 || m > mj::kPatchMaxMerge) { snprintf(why, cap, "merge %d is not 1..%d", m, mj::kPatchMaxMerge); return false; }
    if (t < 1 || t > mj::kPatchMaxRepeat) { snprintf(why, cap, "repeat %d is not 1..%d", t, mj::kPatchMaxRepeat); return false; }
    if (order != MJ_PATCH_CHW && order != MJ_PATCH_HWC) { snprintf(why, cap, "order %d", order); return false; }
    if (order == MJ_PATCH_HWC && t != 1) { snprintf(why, cap, "order hwc needs repeat 1, not %d", t); return false; }
    if (length < 0) { snprintf(why, cap, "length %d is below 0", length); return false; }
    const int64_t block = (int64_t)m * m * ncomp * t * P * P * es;
    if (block > mj::kPatchBlockBytes) {
        snprintf(why, cap, "a merge block of %lld bytes (merge %d, patch %d, repeat %d, %d components of %d bytes), more than %d", (long long)block, m, P, t, ncomp, es,
                 mj::kPatchBlockBytes);
        return false;
    }
    const int mP = m * P;
    for (int k = 0; k < n_sources; ++k) {
        const mj_patch_window q = windows ? windows[k] : mj_patch_window{0, 0, sw, sh};
        auto no = [&](const char *what) {
            snprintf(why, cap, "source %d (%s %d, %d, %d x %d): %s", k, windows ? "window" : "the whole canvas", q.x, q.y, q.width, q.height, what);
            return false;
        };
        if (q.width < 1 || q.height < 1) return no("a width or height below 1");
        if (q.x < 0 || q.y < 0 || (int64_t)q.x + q.width > sw || (int64_t)q.y + q.height > sh) return no("the window is not inside the source canvas");
        if (q.width % mP || q.height % mP) {
            snprintf(why, cap, "source %d (%s %d, %d, %d x %d): width and height must be multiples of patch * merge = %d", k, windows ? "window" : "the whole canvas", q.x,
                     q.y, q.width, q.height, mP);
            return false;
        }
        const int64_t tokens = (int64_t)(q.width / P) * (q.height / P);
        if (length && tokens > length) {
            snprintf(why, cap, "source %d (%s %d, %d, %d x %d): %lld tokens, more than length %d", k, windows ? "window" : "the whole canvas", q.x, q.y, q.width, q.height,
                     (long long)tokens, length);
            return false;
        }
    }
    return true;
}

bool check_arrays(const void *src, const void *dst, int es, int ncomp, int sw, int sh, int n_sources, int64_t rows, int D, char *why, size_t cap) {
    if (!src || !dst) { snprintf(why, cap, "NULL argument"); return false; }
    const uint64_t sslot = (uint64_t)sw * sh * ncomp * es, drow = (uint64_t)D * es;        // (below 2^36, below 2^18)
    if ((uint64_t)n_sources > ((uint64_t)1 << 62) / sslot || (uint64_t)rows > ((uint64_t)1 << 62) / drow) {
        snprintf(why, cap, "%d sources of %llu bytes, %lld rows of %llu bytes: more than an address holds", n_sources, (unsigned long long)sslot, (long long)rows,
                 (unsigned long long)drow);
        return false;
    }
    const uint64_t sbytes = (uint64_t)n_sources * sslot, dbytes = (uint64_t)rows * drow;
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (s % es || d % es) { snprintf(why, cap, "src or dst is not aligned to its %d-byte elements", es); return false; }
    if (s < d + dbytes && d < s + sbytes) { snprintf(why, cap, "src and dst overlap (%llu and %llu bytes)", (unsigned long long)sbytes, (unsigned long long)dbytes); return false; }
    return true;
}

// checked: the jobs of a launch (or of the host twin's walk) and its arguments but for the job pointer
int patch_prepare(mj_context *ctx, const char *fn, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t sw, int32_t sh, int32_t n_sources,
                  int32_t P, int32_t m, int32_t t, int32_t order, int32_t length, const mj_patch_window *windows, std::vector<mj::DevPatchJob> &jobs, mj::PatchArgs *a,
                  mj::PatchGeom *geom) {
    char why[320];
    if (!check_geometry(layout, dtype, ncomp, sw, sh, n_sources, P, m, t, order, length, windows, why, sizeof(why))) return fail(ctx, MJ_ERR_INVALID, "%s: %s", fn, why);
    const mj::PatchGeom g{sw, sh, ncomp, layout, P, m, t, order == MJ_PATCH_HWC, length};
    const mj::PatchWindow *win = reinterpret_cast<const mj::PatchWindow *>(windows);
    const int es = mj::erase_esize(dtype);
    if (!check_arrays(src, dst, es, ncomp, sw, sh, n_sources, mj::patch_rows(g, n_sources, win), mj::patch_D(g), why, sizeof(why)))
        return fail(ctx, MJ_ERR_INVALID, "%s: %s", fn, why);
    mj::patch_jobs(g, es, n_sources, win, jobs);
    if (jobs.size() > (size_t)0x7FFFFFFF) return fail(ctx, MJ_ERR_INVALID, "%s: %zu jobs: more than a launch holds", fn, jobs.size());
    mj::patch_args(g, a);
    a->src = src; a->dst = dst; a->jobs = nullptr; a->n_jobs = (int32_t)jobs.size();
    *geom = g;
    return MJ_OK;
}

// the jobs into the context's device buffer, behind the previous patchify launch (which reads it), ahead of this one on `s`
int stage_patch_jobs(mj_context *ctx, hipStream_t s, const std::vector<mj::DevPatchJob> &jobs) {
    const size_t bytes = jobs.size() * sizeof(mj::DevPatchJob);
    if (ctx->patch_flying) { MJ_HIP(ctx, hipEventSynchronize(ctx->patch_done)); ctx->patch_flying = false; }
    if (!ctx->patch_done) MJ_HIP(ctx, hipEventCreateWithFlags(&ctx->patch_done, hipEventDisableTiming));
    if (bytes > ctx->patch_cap) {
        if (ctx->h_patch) { (void)hipHostFree(ctx->h_patch); ctx->h_patch = nullptr; }
        if (ctx->d_patch) { (void)hipFree(ctx->d_patch); ctx->d_patch = nullptr; }
        ctx->patch_cap = 0;
        const size_t cap = bytes + bytes / 2 + 4096;
        MJ_HIP(ctx, hipHostMalloc(&ctx->h_patch, cap, hipHostMallocDefault));
        MJ_HIP(ctx, hipMalloc(&ctx->d_patch, cap));
        ctx->patch_cap = cap;
    }
    memcpy(ctx->h_patch, jobs.data(), bytes);
    MJ_HIP(ctx, hipMemcpyAsync(ctx->d_patch, ctx->h_patch, bytes, hipMemcpyHostToDevice, s));
    return MJ_OK;
}

template <typename T>
void host_patchify(const T *src, T *dst, const mj::PatchArgs &a, const std::vector<mj::DevPatchJob> &jobs) {
    const int group = a.planar ? 1 : a.C;
    const int64_t s_x = a.rows ? group : a.s_line, s_y = a.rows ? a.s_line : group, s_c = a.planar ? a.s_c : 1;
    for (const mj::DevPatchJob &job : jobs) {
        T *d = dst + job.dst;
        if (job.src < 0) {
            for (int e = 0; e < job.count; ++e) d[e] = (T)0;
            continue;
        }
        const T *s = src + job.src;
        for (int c = 0; c < a.C; ++c)
            for (int yy = 0; yy < a.mP; ++yy)
                for (int xx = 0; xx < job.count * a.mP; ++xx) {
                    const T el = s[c * s_c + yy * s_y + xx * s_x];
                    const int32_t at = mj::patch_index(a, c, yy, xx);
                    for (int r = 0; r < a.t; ++r) d[at + r * a.P * a.P] = el;
                }
    }
}

}  // namespace

extern "C" {

int mj_patchify(mj_context *ctx, void *stream, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height,
                int32_t n_sources, int32_t patch, int32_t merge, int32_t repeat, int32_t order, int32_t length, const mj_patch_window *windows) {
    if (!ctx) return MJ_ERR_INVALID;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    mj::PatchArgs a{};
    mj::PatchGeom g{};
    std::vector<mj::DevPatchJob> jobs;
    if (int rc = patch_prepare(ctx, "mj_patchify", src, dst, layout, dtype, ncomp, src_width, src_height, n_sources, patch, merge, repeat, order, length, windows, jobs, &a,
                               &g))
        return rc;
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = stage_patch_jobs(ctx, s, jobs)) return rc;
    a.jobs = static_cast<const mj::DevPatchJob *>(ctx->d_patch);
    // (the event goes behind the staging copy whether or not the launch went out, as in mj_compose)
    const int es = mj::erase_esize(dtype);
    const hipError_t launched = mj::launch_patchify(s, a, es, mj::patch_lds_bytes(g, es));
    const hipError_t recorded = hipEventRecord(ctx->patch_done, s);
    if (recorded == hipSuccess) ctx->patch_flying = true;
    else (void)hipStreamSynchronize(s);
    MJ_HIP(ctx, launched);
    MJ_HIP(ctx, recorded);
    return MJ_OK;
}

int mj_patchify_time(mj_context *ctx, int iters, const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height,
                     int32_t n_sources, int32_t patch, int32_t merge, int32_t repeat, int32_t order, int32_t length, const mj_patch_window *windows, float *ms_out) {
    if (!ctx || iters <= 0 || !ms_out) return MJ_ERR_INVALID;
    hipStream_t s = ctx->stream;
    mj::PatchArgs a{};
    mj::PatchGeom g{};
    std::vector<mj::DevPatchJob> jobs;
    if (int rc = patch_prepare(ctx, "mj_patchify_time", src, dst, layout, dtype, ncomp, src_width, src_height, n_sources, patch, merge, repeat, order, length, windows, jobs,
                               &a, &g))
        return rc;
    MJ_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = stage_patch_jobs(ctx, s, jobs)) return rc;
    a.jobs = static_cast<const mj::DevPatchJob *>(ctx->d_patch);
    // (the staged jobs are read until the last launch ends: every way out of here leaves the stream drained, so patch_flying stays false)
    struct Drain {
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{s};
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    const int es = mj::erase_esize(dtype);
    const size_t lds = mj::patch_lds_bytes(g, es);
    MJ_HIP(ctx, hipEventCreate(&ev.a));
    MJ_HIP(ctx, hipEventCreate(&ev.b));
    MJ_HIP(ctx, mj::launch_patchify(s, a, es, lds));        // (warm)
    MJ_HIP(ctx, hipEventRecord(ev.a, s));
    for (int i = 0; i < iters; ++i) MJ_HIP(ctx, mj::launch_patchify(s, a, es, lds));
    MJ_HIP(ctx, hipEventRecord(ev.b, s));
    MJ_HIP(ctx, hipEventSynchronize(ev.b));
    float ms = 0.f;
    MJ_HIP(ctx, hipEventElapsedTime(&ms, ev.a, ev.b));
    *ms_out = ms / iters;
    return MJ_OK;
}

int mj_host_patchify(const void *src, void *dst, int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height, int32_t n_sources, int32_t patch,
                     int32_t merge, int32_t repeat, int32_t order, int32_t length, const mj_patch_window *windows) {
    mj::PatchArgs a{};
    mj::PatchGeom g{};
    std::vector<mj::DevPatchJob> jobs;
    if (int rc = patch_prepare(nullptr, "mj_host_patchify", src, dst, layout, dtype, ncomp, src_width, src_height, n_sources, patch, merge, repeat, order, length, windows,
                               jobs, &a, &g))
        return rc;
    switch (mj::erase_esize(dtype)) {
        case 1: host_patchify(static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), a, jobs); break;
        case 2: host_patchify(static_cast<const uint16_t *>(src), static_cast<uint16_t *>(dst), a, jobs); break;
        default: host_patchify(static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), a, jobs); break;
    }
    return MJ_OK;
}

int mj_host_patchify_count(int32_t layout, int32_t dtype, int32_t ncomp, int32_t src_width, int32_t src_height, int32_t n_sources, int32_t patch, int32_t merge,
                           int32_t repeat, int32_t order, int32_t length, const mj_patch_window *windows, int64_t *rows) {
    const char *fn = "mj_host_patchify_count";
    char why[320];
    if (!rows) return fail(nullptr, MJ_ERR_INVALID, "%s: NULL argument", fn);
    if (!check_geometry(layout, dtype, ncomp, src_width, src_height, n_sources, patch, merge, repeat, order, length, windows, why, sizeof(why)))
        return fail(nullptr, MJ_ERR_INVALID, "%s: %s", fn, why);
    const mj::PatchGeom g{src_width, src_height, ncomp, layout, patch, merge, repeat, order == MJ_PATCH_HWC, length};
    *rows = mj::patch_rows(g, n_sources, reinterpret_cast<const mj::PatchWindow *>(windows));
    return MJ_OK;
}

}  // extern "C"
