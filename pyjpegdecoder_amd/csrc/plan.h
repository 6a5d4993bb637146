// Host-side state of libmijpeg.so shared by its translation units: the device buffer cache, the context and the plan
// (api.hip: the C ABI and the launches of an execute; plan_create.hip: mj_plan_create_with; options.hip: the test / tuning switches).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <array>
#include <string>
#include <vector>

#include "mijpeg_internal.h"
#include "form_select.h"
#include "erase_addr.h"

// Device buffers of destroyed plans, kept by the context for the next plan.  A decode service creates one plan per
// batch; hipMalloc / hipFree of its multi-gigabyte coefficient store every time costs more than the decode (the
// runtime hands freed memory back lazily: measured 300-700 ms stalls every few batches of 512 x 1080p), and
// hipFree waits for the device.  Sizes are rounded up to 1/8-octave steps so that batches of similar size reuse each
// other's buffers; the cache is bounded (a quarter of the device's memory, MJ_CACHE_MB overrides) and evicts the
// least recently released buffers.
struct DevBufferCache {
    struct Block { void *ptr; size_t size; uint64_t stamp; };
    std::vector<Block> free_blocks;
    std::vector<Block> live;            // handed out (size needed again at release)
    size_t cached_bytes = 0, limit_bytes = 0;
    uint64_t clock = 0;
    uint64_t n_hit = 0, n_miss = 0, n_evict = 0;    // MJ_CACHE_STATS=1 prints them when the context goes
    uint64_t n_get = 0, size_hash = 0;              // requests so far and a running hash of their sizes, in order (mj_debug_cache_stats)
    static size_t bucket(size_t n) {
        if (n <= 4096) return 4096;
        size_t p2 = (size_t)1 << (63 - __builtin_clzll((unsigned long long)n));
        const size_t step = p2 >> 3;
        return (n + step - 1) / step * step;
    }
    hipError_t get(void **out, size_t bytes) {
        const size_t want = bucket(bytes);
        ++n_get;
        size_hash = size_hash * 0x100000001b3ull + bytes;
        int best = -1;
        for (int i = 0; i < (int)free_blocks.size(); ++i)
            if (free_blocks[i].size == want && (best < 0 || free_blocks[i].stamp > free_blocks[best].stamp)) best = i;
        if (best >= 0) {
            *out = free_blocks[best].ptr;
            cached_bytes -= want;
            ++n_hit;
            free_blocks.erase(free_blocks.begin() + best);
        } else {
            ++n_miss;
            hipError_t e = hipMalloc(out, want);
            if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); trim(0); e = hipMalloc(out, want); }
            if (e != hipSuccess) return e;
        }
        live.push_back({*out, want, 0});
        return hipSuccess;
    }
    // takes ptr off the list of blocks handed out; false: not one of ours
    bool take(void *ptr, Block *b) {
        for (size_t i = 0; i < live.size(); ++i)
            if (live[i].ptr == ptr) { *b = live[i]; live[i] = live.back(); live.pop_back(); return true; }
        return false;
    }
    void put(void *ptr) {
        Block b;
        if (!take(ptr, &b)) { (void)hipFree(ptr); return; }
        b.stamp = ++clock;
        free_blocks.push_back(b);
        cached_bytes += b.size;
        trim(limit_bytes);
    }
    // hand a live block back to the device instead of keeping it for the next plan (mj_plan_tune_placement's losing candidates)
    void drop(void *ptr) { Block b; (void)take(ptr, &b); (void)hipFree(ptr); }
    void trim(size_t keep) {
        while (cached_bytes > keep && !free_blocks.empty()) {
            int old = 0;
            for (int i = 1; i < (int)free_blocks.size(); ++i)
                if (free_blocks[i].stamp < free_blocks[old].stamp) old = i;
            (void)hipFree(free_blocks[old].ptr);
            ++n_evict;
            cached_bytes -= free_blocks[old].size;
            free_blocks.erase(free_blocks.begin() + old);
        }
    }
};

struct mj_context {
    int device = 0;
    hipStream_t stream = nullptr;
    // plan creation clears a plan's big buffers here, beside whatever the context stream is running (another plan's
    // kernels, in a serving loop); the plan's first use waits for its `ready` event
    hipStream_t setup_stream = nullptr;
    // pinned staging for a plan's small uploads (descriptors, tables, segment lists: a few MB), so that they too are
    // queued on the setup stream instead of each blocking the host behind whatever the copy engine is busy with (in a
    // serving loop: the next batch's 300 MB of files).  A plan holds one arena until it is destroyed.
    struct Arena { char *base = nullptr; size_t cap = 0, used = 0; };
    std::vector<Arena> free_arenas;
    Arena *cur = nullptr;          // the arena of the plan being created
    int32_t *h_word = nullptr;     // pinned: where a stream hands one counter to the host (a pageable target would make the
                                   // copy synchronous for the whole device, i.e. wait for other plans' kernels on other streams)
    double *d_idct_tt = nullptr;   // [u*8+v][x*8+y], the reference's InverseDCT.idct_table transposed
    uint8_t *d_dump = nullptr;     // stage 2's dump lines (mj::kStage2DumpBytes)
    bool no_graph = false;         // MJ_NO_GRAPH at context creation: never replay captured graphs
    // Fused launches (fused.hip) of one context take turns: a fused workgroup wants a CU's whole LDS, so two plans' fused
    // launches on two streams cannot share the chip — left to the hardware queues they interleave workgroup by workgroup and
    // both finish later than one after the other would (three plans in flight: 6.58 ms per step against 5.74, round 5).  An
    // execute that contains a fused launch waits — its stream does, not the host — for the context's previous one.
    hipEvent_t fused_done = nullptr;
    hipStream_t fused_stream = nullptr;     // where the latest fused execute went (null: none yet)
    // mj_mix (mix.hip), the one launch that belongs to a call and not to a plan: its per-output records go through a pinned block
    // into a device block, both the context's; a call waits for the previous launch (mix_done) before it rewrites them
    void *h_mix = nullptr, *d_mix = nullptr;
    size_t mix_cap = 0;
    hipEvent_t mix_done = nullptr;
    bool mix_flying = false;
    // mj_compose (compose.hip), the other launch of a call: its job list goes the same way through blocks and an event of its own
    void *h_compose = nullptr, *d_compose = nullptr;
    size_t compose_cap = 0;
    hipEvent_t compose_done = nullptr;
    bool compose_flying = false;
    // mj_patchify (patch.hip), likewise
    void *h_patch = nullptr, *d_patch = nullptr;
    size_t patch_cap = 0;
    hipEvent_t patch_done = nullptr;
    bool patch_flying = false;
    DevBufferCache cache;
    std::string err;
};

extern std::string g_create_err;     // what mj_last_error(NULL) returns (api.hip)

struct mj_plan {
    mj_context *ctx = nullptr;
    // every device block the plan holds from ctx->cache, in the order it took them (alloc / upload below enter them;
    // mj_plan_destroy returns the list).  The typed d_* fields further down only name them for the kernels' arguments.
    std::vector<void *> blocks;
    // `old`'s entry now names `now` (mj_plan_tune_placement: a better-placed block)
    void swap_block(void *old, void *now) { std::replace(blocks.begin(), blocks.end(), old, now); }
    int32_t n_images = 0;
    int32_t layout = 0;
    uint32_t flags = 0;
    int hmax = 1, vmax = 1, ncomp = 3;
    int lut_slots = 1;
    bool uniform = false;
    // row-major plans run the fast stage 2 on the transposed problem: blocks and tables are then stored [u][v]
    bool transposed = false;
    bool generic = false;              // a sampling layout outside the common ones: wave form of stage 1, k_reconstruct_generic
    uint8_t *d_rgb_tmp = nullptr;  // planar layouts: the interleaved image stage 2 writes before the components are separated
    int64_t max_pixels = 0;        // largest width*height of the batch
    int32_t mcus_per_image = 0;
    mj_plan_info info{};
    std::vector<mj::DevImage> h_images;
    // device
    uint8_t *d_blob_owned = nullptr;
    const uint8_t *blob_src = nullptr;  // a caller's device blob that every execute copies into d_blob_owned first (wave form behind
    int64_t blob_src_len = 0;           // MJ_FLAG_GPU_SEGMENT: the kernel reads further ahead than that flag makes the caller pad)
    const uint8_t *d_blob = nullptr;
    mj::DevSegment *d_segs = nullptr;
    int64_t n_segs = 0;
    mj::DevImage *d_images = nullptr;
    mj::DevHuff *d_huff = nullptr;
    uint16_t *d_lut11 = nullptr;        // [n_huff][2048] primary LUTs of the lane-parallel stage-1 kernel
    // resolved 13-bit AC tables of the lane form's fast variant (huffman_lanes13.hip), when the batch's tables fit LDS that way
    int32_t *d_by_length = nullptr;     // restart segments, longest first (how the lane form deals them out to its waves)
    int seg_order_mode = 0;
    uint32_t *d_lut13 = nullptr;        // [n_ac13][8192]
    uint32_t *d_lut12 = nullptr;        // a fused launch's AC tables: back to back, 12-bit main levels (13 where it says so)
    int lutf_off[4] = {0, 0, 0, 0}, lutf_bits[4] = {12, 12, 12, 12}, lutf_total = 0;   // ... byte offset and index bits per LDS slot, bytes in all
    int n_ac13 = 0, n_dc13 = 0;
    uint64_t ac_slot_pk = 0, dc_slot_pk = 0, dc_tab_pk = 0;
    // batches with more tables than LDS holds (files with their own optimised tables): per workgroup, the tables its
    // units of work use — one list for the lane kernel's launch, one for the counting rounds (256 chunks per workgroup)
    int32_t *d_wg_tabs_lanes = nullptr, *d_wg_tabs_count = nullptr;
    int wg_slots_lanes = 0, wg_slots_count = 0;      // 8 or 16 LUTs per workgroup
    uint32_t *d_stream = nullptr;       // stage 0 output (destuff.hip): big-endian dwords per restart segment
    size_t stream_bytes = 0;            // ... its size (mj_plan_tune_placement tries other buffers of that size)
    int32_t *d_seg_bits = nullptr;      // [n_segs] bits per segment after stage 0
    // long restart segments (files without DRI): synchronisation passes + virtual segments (huffman_sync.hip)
    bool use_sync = false;
    int sync_rounds = 32;          // repair rounds of the synchronisation form queued per execute (MJ_SYNC_ROUNDS at plan creation: tests).
                                   // A round behind one that changed nothing returns at once, so the number only bounds the longest
                                   // chain of wrongly guessed entry states that still settles (flat image regions re-synchronise badly:
                                   // round 4 found a quarter of a synthetic batch's images unconverged after four rounds, none after six; an idle round costs ~2 us)
    int sync_chunk_bytes = 2048;
    int sync_warm_bits = -1;       // run-up in front of every chunk of the counting rounds (MJ_SYNC_WARM at plan creation; -1 = half a chunk)
    uint16_t *d_lut11u = nullptr;       // every table as len << 11 | run << 4 | size
    mj::DevChunk *d_chunks = nullptr;
    int64_t n_chunks = 0;
    uint64_t *d_stateA = nullptr, *d_stateB = nullptr;
    mj::DevChunkOut *d_couts = nullptr;
    mj::DevVSeg *d_vsegs = nullptr;
    int32_t *d_seg_chunk0 = nullptr;    // [n_segs + 1] first chunk of every restart segment
    uint32_t *d_lutc = nullptr;         // the counting walks' resolved tables (k_count), or null: the classic rounds (k_sync_count)
    int lutc_tab_bytes = 0, lutc_bits = 0;
    void *d_sync_items = nullptr;       // the repair launch's work list (16 bytes per chunk); its counter is d_changed[0]
    hipGraphExec_t graph_exec = nullptr;   // captured launches of one execute (see mj_plan_execute)
    hipStream_t graph_stream = nullptr;
    uint8_t *graph_rgb = nullptr;
    bool executed_once = false;
    mj_context::Arena arena;               // pinned staging of this plan's uploads (back to the context at destroy)
    hipEvent_t ready = nullptr;             // recorded behind the creation-time clears on the context's setup stream
    bool ready_done = false;
    hipStream_t ready_stream = nullptr;     // the stream that was made to wait for `ready`
    hipEvent_t done = nullptr;              // recorded behind the plan's latest execute: what mj_plan_sync / _read / _destroy wait for
    bool done_valid = false;
    bool last_was_graph = false;
    hipStream_t prev_stream = nullptr;      // of the last plain execute
    uint8_t *prev_rgb = nullptr;
    mj::DevPiece *d_pieces = nullptr;   // stage 0 of long segments, piece by piece
    int64_t n_pieces = 0;
    int32_t *d_piece_kept = nullptr;
    int32_t *d_changed = nullptr;
    mj::DevScanJob *d_jobs = nullptr;   // MJ_FLAG_GPU_SEGMENT: per-image byte ranges for the marker scan
    int n_jobs = 0;
    int n_huff = 0;
    bool use_lanes = false;
    // stages 1 + 2 in one launch (fused.hip) for mj_plan_execute, where the batch is of the kind it takes
    bool use_fused = false;
    mj::FusedShape fused{};
    int fused_spi = 0;                  // restart segments (= MCU rows) per image
    int32_t *d_holder = nullptr;        // fused, segments dealt out by length: per segment, the progress word of the wave that walks it
    uint32_t *d_xwords = nullptr;       // ... the launch's ticket counter (32 words: a line of its own) and the progress words
    // progressive batches: scans grouped by dependency level, one launch per level
    bool progressive = false;
    mj::DevProgScan *d_pscans = nullptr;
    mj::DevProgSeg *d_psegs = nullptr;
    mj::DevProgState *d_pstates = nullptr;   // per segment: what a scan carries from band to band
    int64_t n_psegs = 0;
    int prog_rows_per_band = 2, prog_steps = 0;
    bool prog_banded = false;
    // the first scans and the refining AC scans read the stage-0 stream of the scans' segments (progressive_fast.hip)
    mj::DevSegment *d_prog_dsegs = nullptr;  // d_psegs' byte ranges in the form stage 0 takes
    uint16_t *d_lut11p = nullptr;            // [n_huff][1 << kProgLutBits], (len << 8 | symbol)
    bool prog_fast = false;
    int64_t prog_rest_off = 0;               // banded: d_psegs[prog_rest_off..] are the segments of the scans progressive.hip walks
    mj::DevProgSub *d_psubs = nullptr;       // [n_split][2][kProgSub]: by segment, two sets (even and odd bands)
    int prog_parts = 4;                      // ... parts per band
    // the first AC scans of large batches in chunks (progressive_chunks.hip): d_psegs[n_psegs_wave..] are theirs, no wavefront walk takes them
    bool prog_chunks = false;
    int pc_chunk_bytes = 512;
    int64_t n_psegs_wave = 0;
    mj::DevAcSeg *d_acsegs = nullptr;
    int n_acsegs = 0;
    mj::DevChunk *d_pc_chunks = nullptr;
    int64_t n_pc_chunks = 0;
    uint8_t *d_pc_tabs = nullptr;
    uint64_t *d_pc_exit = nullptr;
    mj::DevChunkOut *d_pc_outs = nullptr;
    void *d_pc_items = nullptr;
    int32_t *d_pc_owner = nullptr;
    mj::DevVSeg *d_pc_vsegs = nullptr;
    int64_t n_split = 0;                     // banded: d_psegs[0..n_split) are the segments of the scans walked as scout + parts
    // (one launch per dependency level only — MJ_PROG_BANDS=0; the band pipeline orders d_psegs by length instead)
    std::vector<int64_t> ordinal_seg_off;   // [n_ordinals + 1] into d_psegs
    std::vector<int64_t> ordinal_kind_off;  // [n_ordinals][4]: within a level, where the segments of each kind of scan start
    uint16_t *d_qt = nullptr;
    int64_t *d_mcu_prefix = nullptr;
    int64_t *d_job_prefix = nullptr;    // fast stage 2: first job of every image (+ total), then the kernel's ticket counter
    int64_t total_jobs = 0;
    int32_t jobs_per_image = 0;
    int32_t chunk_strips = 16;          // strips per job (a piece of one MCU column) of the fast stage 2
    int32_t jobs_per_ticket = 1;        // consecutive jobs a wave draws at once
    int16_t *d_tmp_coef = nullptr;      // staging for zig-zag <-> natural conversion
    int16_t *d_coef = nullptr;
    uint8_t *d_rgb = nullptr;       // plan-owned, allocated on first use
    int16_t *d_planes = nullptr;
    int16_t *d_idct = nullptr;
    int32_t *d_status = nullptr;
    uint8_t *last_rgb = nullptr;    // where the most recent execute wrote
    // window plans (mj_plan_request.rois): per image the window stage 2 writes; the exact-order and generic kernels number the
    // windows' MCUs (win_mcu_prefix: first window MCU of every image + total)
    bool windowed = false;
    std::vector<mj::DevWindow> h_win;
    mj::DevWindow *d_win = nullptr;
    int64_t *d_win_mcu_prefix = nullptr;
    int64_t win_total_mcus = 0;
    // ... of MJ_FLAG_GPU_SEGMENT batches: the marker scan fills every restart segment of the images here, and the ones the
    // windows need are gathered (d_seg_gather: their indices) into d_segs, which stages 0 and 1 read
    mj::DevSegment *d_segs_full = nullptr;
    int32_t *d_seg_gather = nullptr;
    // resized plans (mj_plan_request.out_width / out_height): stage 2 writes its interleaved pixels into d_src, the resize launch reads them and
    // writes the plan's output (info.rgb_bytes is the OUTPUT's size; src_bytes the intermediate's)
    bool resized = false;
    uint8_t *d_src = nullptr;
    int64_t src_bytes = 0;
    mj::DevResizeImage *d_rz_images = nullptr;
    int32_t *d_rz_tabs = nullptr;
    uint8_t *d_rz_mirror = nullptr;        // ... with a mirror flag set: one byte per image
    uint8_t *d_rz_lut = nullptr;           // mj_plan_request.output with a float dtype: the output table (info.rgb_bytes: bytes of that type)
    mj::ResizeArgs rz{};
    int rz_placed = 0;                     // mj_plan_request.places: the placed instances, which store rz_fill (byte c in bits
    unsigned rz_fill = 0;                  // 8c..8c+7) where an image does not cover the canvas
    int rz_filter = 0, rz_max_ksize = 0;   // the plan's MJ_FILTER_* and the most taps a pixel of it has per axis (mj_debug_resize_shape)
    // reducing plans (mj_plan_request.reducing_gap with a factor above 1 somewhere): the reduce launch (reduce.hip) between stage 2
    // and the resize launch reads d_src and writes the reduced images, packed, into d_red, which is what rz.src then names
    bool reduces = false, rd_luma = false;     // rd_luma: colour to L is the reduce launch's; the resize runs the one-component instances
    uint8_t *d_red = nullptr;
    mj::DevReduceImage *d_rd_images = nullptr;
    mj::ReduceArgs rd{};
    // plans with an affine transform (mj_plan_request.affine): the affine launch (affine.hip) between stage 2 and the resize launch reads
    // d_src and writes every output's window of its transformed image, packed, in the output's components (af_ncomp), into d_aff,
    // which is what rz.src then names; the resize launch runs the plain instances of af_ncomp components on upright records
    bool affine = false;
    int af_ncomp = 0;
    int64_t af_bytes = 0;
    uint8_t *d_aff = nullptr;
    mj::DevAffineImage *d_af_images = nullptr;
    int32_t *d_af_tabs = nullptr;
    mj::AffineArgs af{};
    // ... or a perspective transform (mj_plan_request.perspective): `affine` is set, the buffer and af_* are as above, and the launch is
    // the perspective one with records of its own
    bool perspective = false;
    mj::DevPerspectiveImage *d_pf_images = nullptr;
    mj::PerspectiveArgs pf{};
    // plans with colour operations (mj_plan_request.colour): the resize launch writes uint8 canvases, unmirrored,
    // output after output, into the first half of d_canvas; the colour launches (colour.hip) take them through their chains, from one
    // half to the other, and store the last step into the caller's array — slots, mirror flags and the output table are theirs.
    // d_blur_scratch: a third canvas, only on plans that blur pass by pass (co_blur.lds == 0 with a blur in some chain)
    bool colour = false;
    uint8_t *d_canvas = nullptr;
    uint8_t *d_blur_scratch = nullptr;
    uint32_t *d_blur_weights = nullptr;         // ww and fw of every blur op (ColourBlurArgs::weights), only on plans with a blur
    uint32_t *d_co_hist = nullptr;
    uint8_t *d_co_tables = nullptr;
    mj::DevColourOutput *d_co_outputs = nullptr;
    int32_t *d_co_list = nullptr;
    mj::HueTables *d_hue_tables = nullptr;      // colour_hue_tables() (ColourHueArgs::tables), only on plans with a hue launch
    mj::ColourArgs co{};
    mj::ColourBlurArgs co_blur{};
    mj::ColourHueArgs co_hue{};
    // erase (mj_plan_set_erase): boxes of the finished outputs overwritten by one more launch — or one per box ordinal where boxes of
    // one output intersect — behind everything else resize_launch queues (erase.hip).  What a sized plan's maker leaves for it:
    // the output's components and MJ_DTYPE_*, the array's slots and every output's slot (h_slot); what the call leaves: the
    // records and job list (plan-owned), the caller's values and the launches as [first job, jobs]
    int er_C = 0, er_dtype = 0, er_slots = 0;
    std::vector<int32_t> h_slot;
    mj::DevEraseRect *d_er_rects = nullptr;
    mj::DevEraseJob *d_er_jobs = nullptr;
    const void *er_values = nullptr;
    std::vector<std::array<int32_t, 2>> er_launches;
    int64_t er_bytes = 0;                      // bytes the launches write
    int32_t n_views = 0;                       // a plan with views (mj_plan_request.views): its resize and reduce records are per view (0: per image)
    std::vector<std::array<int32_t, 2>> h_view_size;   // ... every view's window, stored axes: width, height (mj_debug_reduce_shape)
    std::vector<std::array<int32_t, 6>> h_rd;  // per image (view), stored axes: fx, fy, phase x, phase y, reduced width, height (mj_debug_reduce_shape)
    // oriented plans at the files' own sizes (mj_plan_request.orientations without a size): `resized` with the orient launch (orient.hip) in the
    // resize launch's place — stage 2 writes stored-order pixels into d_src, the launch writes them oriented into the output
    bool orient_only = false;
    mj::DevOrientImage *d_or_images = nullptr;
    int64_t *d_or_prefix = nullptr;
    mj::OrientArgs oa{};
    // plans that convert (mj_plan_request.mode): the components of the output where they are not the
    // files' (0: they are) — the orient / resize launch converts —, and every image's byte offset in the output
    int out_ncomp = 0;
    std::vector<int64_t> h_out_off;
    // plans are counted: the caller holds one reference until mj_plan_destroy, and every derived plan (mj_plan_derive) holds one to
    // its parent.  The device blocks and the arena go back to the context with the last reference; mj_plan_destroy itself waits for
    // the plan's own events and gives them up.
    int refs = 1;
    // derived plans: only the launches behind the decode (resize_launch), over the parent's d_src, which this plan names and does
    // not own.  No blob, no coefficient store, no statuses: the decode's entry points refuse it.
    bool derived = false;
    mj_plan *parent = nullptr;
};

// ---- plan_tables.hip: table building (host)
namespace mj {
// DHT -> canonical code book + 9-bit LUT (jpeg_decoder.py:366-377)
void build_dev_huff(const mj_huff_spec &spec, DevHuff &h);
bool build_resolved_tables(const mj_batch *b, const std::vector<int> &role, uint64_t ac_pk, int n_ac, const int ab_of_slot[4], int fixed_slot_bytes,
                           std::vector<uint32_t> &out, int slot_off[4], int &total_bytes);
bool build_count_tables(const mj_batch *b, const std::vector<int> &role, int W, std::vector<uint32_t> &out, int &tab_bytes);
// ---- plan_progressive.hip: the progressive side of mj_plan_create
struct ProgScans { std::vector<DevProgScan> pscans; std::vector<DevProgSeg> psegs; };
int plan_progressive_scans(mj_context *ctx, const mj_batch *b, mj_plan *p, ProgScans &S, int64_t &entropy_bytes);
int plan_progressive_upload(mj_context *ctx, const mj_batch *b, mj_plan *p, ProgScans &S);
// ---- plan_create.hip: the plain plan and the window plan (roi_plan; rois == NULL: every window is the whole image)
int plan_create_common(mj_context *ctx, const mj_batch *b, const mj_roi *rois, bool roi_plan, mj_plan **out);
// What mj_plan_create_with is asked for, after plan_create.hip's normalise_request: every field of r is checked, and one that
// named its default names nothing (orientations all 1, the batch's own mode, every place the whole canvas: NULL / 0); n_slots
// is the output's.  The two makers take it: create_resized (resize_plan.hip) with a size, create_oriented (orient.hip) without
// one and with orientations or a mode; a request with neither is plan_create_common's.
// r.views: r.n_views entries where r.n_views != 0, else NULL
// r.affine / r.perspective: one entry per output where some output is transformed, else NULL — at most one of the two, and
// without either r.transform_filter and r.transform_fill are 0.  Such a request ALWAYS has views after normalisation: its
// windows (r.rois) or whole images become one view per image, held in own_views, which r.views then names
// r.colour: one chain per output where some chain is not empty, else NULL
struct PlanRequest {
    mj_context *ctx; const mj_batch *b; mj_plan **out; mj_plan_request r;
    std::vector<mj_view> own_views{};
};
// an output without a transform: all six entries 0
inline bool affine_none(const mj_affine &m) { return !m.a[0] && !m.a[1] && !m.a[2] && !m.a[3] && !m.a[4] && !m.a[5]; }
inline bool perspective_none(const mj_perspective &m) {
    for (double v : m.a)
        if (v) return false;
    return true;
}
constexpr const char *kCreateFn = "mj_plan_create_with";     // (for the messages)
int create_resized(const PlanRequest &q);
// mj_plan_derive's maker (resize_plan.hip): the stages of a sized request on a shell plan that reads `parent`'s decoded images
int create_derived(const PlanRequest &q, mj_plan *parent);
// reducing_gap's default rule (normalise_request): whether any image of the request — oriented, its window, to its place's size —
// gets a factor above 1; images whose sizes the makers will refuse count as none
bool reduce_applies(const mj_batch *b, const mj_plan_request &r);
const char *output_fault(int dtype, bool normalize, int ncomp, const float *mean, const float *std);     // (resize_plan.hip)
int create_oriented(const PlanRequest &q);
// ---- erase.hip: the erase launches of one execute (mj_plan_set_erase), behind everything else it queued on s; none set: nothing
int erase_execute(mj_plan *p, hipStream_t s);
// q.r.rois (oriented coordinates, not NULL) or the windows `rois` given in their place, as windows of the stored images
int stored_windows(const PlanRequest &q, const mj_roi *rois, std::vector<mj_roi> &stored);
// destroys a plan under construction unless its maker got to the end (p = nullptr)
struct PlanGuard { mj_plan *p; ~PlanGuard() { if (p) mj_plan_destroy(p); } };
// ---- EXIF orientation (tools/orient_model.py): value 1..8 as operations on the row-major image — bit 2: transpose first,
// then bit 0: reverse the columns, bit 1: reverse the rows
inline int orient_bits(int o) {
    static const int bits[9] = {0, 0, 1, 3, 2, 4, 5, 7, 6};
    return bits[o];
}
// the window of the stored width x height image that window r of the oriented image shows (orient_model.stored_window);
// false: r is empty or not inside the oriented image
inline bool stored_window(int o, int width, int height, const mj_roi &r, mj_roi *out) {
    const int bits = orient_bits(o);
    const int64_t wo = (bits & 4) ? height : width, ho = (bits & 4) ? width : height;
    if (r.width <= 0 || r.height <= 0 || r.x < 0 || r.y < 0 || (int64_t)r.x + r.width > wo || (int64_t)r.y + r.height > ho) return false;
    const int x = (bits & 1) ? (int)(wo - r.x - r.width) : r.x, y = (bits & 2) ? (int)(ho - r.y - r.height) : r.y;
    *out = (bits & 4) ? mj_roi{y, x, r.height, r.width} : mj_roi{x, y, r.width, r.height};
    return true;
}
// view v of a request with views: its window of the oriented image (`shown`; a window that is all zero: the whole of it) and
// the window of the stored image that shows (`stored`); false: the window is empty or not inside the oriented image
inline bool view_window(const mj_batch *b, const uint8_t *orient, const mj_view &v, mj_roi *shown, mj_roi *stored) {
    const mj_image_desc &im = b->images[v.image];
    const int o = orient ? orient[v.image] : 1;
    *shown = v.window;
    if (!v.window.x && !v.window.y && !v.window.width && !v.window.height) {
        const bool t = (orient_bits(o) & 4) != 0;
        *shown = mj_roi{0, 0, t ? im.height : im.width, t ? im.width : im.height};
    }
    return stored_window(o, im.width, im.height, *shown, stored);
}
}  // namespace mj

// (one definition per translation unit: they return through the caller's frame)
namespace {

int fail(mj_context *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_err = buf;
    return code;
}

#define MJ_HIP(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((ctx), MJ_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// a device buffer of the plan's, from its context's cache
template <typename T>
hipError_t alloc(mj_plan *p, T **dst, size_t bytes) {
    if (*dst) {         // a field that holds a block already (fused_tables' second try) gives it back first
        p->ctx->cache.put(*dst);
        p->blocks.erase(std::find(p->blocks.begin(), p->blocks.end(), (void *)*dst));
        *dst = nullptr;
    }
    const hipError_t e = p->ctx->cache.get((void **)dst, bytes);
    if (e == hipSuccess) p->blocks.push_back(*dst);
    return e;
}

// a host array into such a buffer — through the plan's pinned arena on the setup stream where it fits
template <typename T>
int upload(mj_plan *p, T **dst, const T *src, size_t n, size_t pad_bytes = 0) {
    mj_context *ctx = p->ctx;
    MJ_HIP(ctx, alloc(p, dst, n * sizeof(T) + pad_bytes + 16));
    if (pad_bytes) MJ_HIP(ctx, hipMemsetAsync((char *)*dst + n * sizeof(T), 0, pad_bytes, ctx->setup_stream));
    const size_t bytes = n * sizeof(T);
    if (!bytes) return MJ_OK;
    mj_context::Arena *a = ctx->cur;
    const size_t at = a ? (a->used + 63) & ~(size_t)63 : 0;
    if (a && at + bytes <= a->cap) {
        memcpy(a->base + at, src, bytes);
        a->used = at + bytes;
        MJ_HIP(ctx, hipMemcpyAsync(*dst, a->base + at, bytes, hipMemcpyHostToDevice, ctx->setup_stream));
    } else {
        MJ_HIP(ctx, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));      // big (a host blob) or no arena: the plain way
    }
    return MJ_OK;
}

}  // namespace
