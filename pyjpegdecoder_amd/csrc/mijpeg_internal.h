// Internal device/host structures of libmijpeg.so (gfx950 only).
#pragma once
#include <atomic>
#include <mutex>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mijpeg.h"

namespace mj {

constexpr int kWave = 64;               // CDNA4 wavefront
constexpr int kLutBits = 9;             // primary Huffman LUT: codes up to 9 bits resolve in one LDS read
constexpr int kLutSize = 1 << kLutBits;
constexpr int kMaxBlocksPerMcu = 16;    // the common layouts have <= 6 (4:2:0 = 4 Y + Cb + Cr); T.81 allows 10 per interleaved scan, the reference does not check (:774-785)
constexpr int kMaxTabsPerImage = 6;     // DC+AC for up to three components

// One Huffman table on the device.  `lut` is staged into LDS by the stage-1 kernel; the long-code
// side (codes of 10..16 bits, a few percent of symbols) stays in global memory / L2.
struct DevHuff {
    uint16_t lut[kLutSize];   // (len << 8) | symbol for codes <= kLutBits bits, 0 = longer code
    int32_t first_code[17];   // canonical code book per length (jpeg_decoder.py:366-377)
    int32_t count[17];
    int32_t first_sym[17];
    uint8_t vals[256];
    uint8_t pad[4];
};
static_assert(sizeof(DevHuff) % 8 == 0, "DevHuff must keep 8-byte alignment in arrays");

// Per-image description used by both kernels.
struct DevImage {
    int32_t width, height, ncomp;
    int32_t hmax, vmax;               // MCU = (8*hmax) x (8*vmax) pixels
    int32_t blocks_per_mcu;
    int32_t mcu_count_h, mcu_count_v;
    int32_t restart_interval;
    int32_t n_tabs;                   // distinct Huffman tables of this image (<= kMaxTabsPerImage)
    int32_t tab_index[kMaxTabsPerImage];   // indices into the batch's DevHuff array
    // for each block of an MCU, in decode order (jpeg_decoder.py:774, :805):
    // (the common layouts have at most 6 blocks per MCU and the lane / synchronisation forms read the first 8 entries as one
    // 64-bit word; layouts with more blocks — kMaxBlocksPerMcu — are decoded by the wave form and k_reconstruct_generic)
    uint8_t blk_comp[kMaxBlocksPerMcu];     // component 0..2
    uint8_t blk_dc_slot[kMaxBlocksPerMcu];  // slot (0..n_tabs-1) of its DC table in the wave's LDS copy
    uint8_t blk_ac_slot[kMaxBlocksPerMcu];
    int32_t qt_index[3];              // per component, into the batch's quantisation tables
    uint8_t comp_h[4], comp_v[4];     // sampling factors per component (jpeg_decoder.py:205-207)
    uint8_t comp_first[4];            // first block of the component inside an MCU
    int32_t generic;                  // 1 = a layout outside the common ones: any factors 1..4 per component
    int32_t pad0;
    int64_t block_off;                // first coefficient block of this image in the packed coef array
    int64_t mcu_off;                  // first MCU of this image in the batch-wide MCU numbering
    int64_t rgb_off;                  // byte offset of this image in the packed RGB output
    int64_t pix_off;                  // pixel offset (for the planes output: *ncomp int16 each)
};

// One image's window of a window plan (mj_plan_request.rois), in the ORIGINAL image's coordinates (x along the width).  The
// image's output (DevImage::rgb_off, in the packing of the windows) is that window only; stage 2 reconstructs the MCUs of
// the window's MCU rectangle and nothing else.
struct DevWindow {
    int32_t x0, y0, w, h;             // pixels: [x0, x0 + w) x [y0, y0 + h)
    int32_t mx0, my0, mcw, mch;       // MCU rectangle: first MCU column / row, MCU columns / rows
};

// One restart segment = the unit of work of one stage-1 wavefront.
struct DevSegment {
    int64_t begin;        // blob offset of the first entropy-coded byte
    int32_t len;          // bytes up to the terminating marker
    int32_t image;
    int32_t mcu0;         // first MCU (within the image) of the segment
    int32_t n_mcu;
    int32_t last;         // 1 = last segment of its image (trailing bytes are not a desync)
    int32_t pad;
};

// One image's byte range for the on-GPU restart-marker scan (MJ_FLAG_GPU_SEGMENT, destuff.hip)
struct DevScanJob {
    int64_t begin, end;   // blob offsets: first entropy-coded byte, a bound at or behind the end of the scan
    int64_t first_seg;    // index of the image's first DevSegment
    int32_t n_seg;        // ceil(mcu_count / restart_interval), 1 without restart interval
    int32_t image;
};

// One chunk of a restart segment's stage-0 stream (huffman_sync.hip): the unit of the synchronisation passes that
// find, inside long segments (files without restart markers), places where an independent decoder can start.
struct DevChunk {
    int32_t seg;          // index of the DevSegment
    int32_t j;            // chunk number within the segment: bits [j * cbits, (j + 1) * cbits)
};
// One piece of a long restart segment for stage 0 (destuff.hip): `len` source bytes from byte `off` of the segment
struct DevPiece {
    int32_t seg;
    int32_t first;        // index of the segment's first piece
    int32_t off, len;
};
// What a counting pass learns about a chunk, decoded from the entry state its predecessor handed over.
struct DevChunkOut {
    uint64_t entry;       // the entry state this record was computed from (a later round skips the chunk if unchanged)
    int32_t blocks;       // blocks completed in the chunk
    int32_t bnd_pos;      // bit position of the first MCU boundary inside the chunk, -1 if none
    int32_t bnd_blocks;   // blocks completed before that boundary
    int16_t dc_bnd[3];    // DC differences per component summed up to the boundary (int16 wrap, :818-820)
    int16_t dc_sum[3];    // ... over the whole chunk
};
static_assert(sizeof(DevChunkOut) == 32, "DevChunkOut layout");
// A virtual segment: a run of whole MCUs inside a restart segment with everything a decoder needs to start there.
struct DevVSeg {
    uint32_t voff0;       // byte offset of the parent segment's stream in the stage-0 buffer
    int32_t bit0, bit_end;    // first bit, one past the last bit (relative to the parent segment's stream)
    int32_t image, mcu0, n_mcu;
    int16_t pred[3];      // DC predictors at the first MCU
    int16_t last;         // 1 = runs to the end of its restart segment (padding bits may follow)
};
static_assert(sizeof(DevVSeg) == 32, "DevVSeg layout");

// One SOS of a progressive image (device copy of mj_scan_desc with table indices resolved).
struct DevProgScan {
    int32_t image, n_comp;
    int32_t comp[3];
    int32_t dc_tab[3], ac_tab[3];   // indices into the batch's DevHuff array
    int32_t ss, se, ah, al;
    int32_t mcu_count_h, mcu_count_v;
    int32_t level;                  // dependency level: scans of level L need the same rows of level L - 1 scans done
    int32_t split;                  // 1: a refining AC scan walked twice (progressive_fast.hip): a scout that only follows the bit
                                    // position, and — one launch behind, at level + 1 — a few walks per band that place
};

// What a scan's restart segment carries from one band of MCU rows to the next (progressive.hip).
struct DevProgState {
    uint64_t bb;
    int32_t pos, bc, pad;
    int32_t eobrun;
    int32_t pred[3];
    int32_t err;
    int32_t mcu_next;               // first MCU the next band starts with
    int32_t reserved;
};

// Where a split scan's scout stood at the first MCU of a part of a band (progressive_fast.hip): what the part's walk starts from.
struct DevProgSub {
    int32_t pos, eobrun, err;
    int32_t mcu;                    // the MCU this entry belongs to (bands alternate between two sets of entries: a stale one does not match)
};
constexpr int kProgSub = 8;         // parts per band: at most (entries per band and segment)

// One restart segment of one progressive scan.
struct DevProgSeg {
    int64_t begin;
    int32_t len;
    int32_t scan;         // index into the DevProgScan array
    int32_t mcu0, n_mcu;  // in units of the scan's own MCUs
    int32_t last;
    int32_t stream_slot;  // the segment's number in stage 0's stream buffer (progressive_fast.hip), blob order
};

}  // namespace mj

namespace mj {
// the first scans and the refining AC scans (progressive_fast.hip) read the stage-0 stream (destuff.hip) of the scans' segments — segment
// number DevProgSeg::stream_slot — and LUTs of kProgLutBits bits, (len << 8 | symbol) per entry, for every table
constexpr int kProgLutBits = 11;
hipError_t launch_progressive_fast(hipStream_t stream, const uint32_t *dstream, const int32_t *seg_bits, const DevProgSeg *segs,
                                   int n_segs, const DevProgScan *scans, const DevImage *images, const DevHuff *huff,
                                   const uint16_t *lut11p, int16_t *coef, int32_t *status, int spec_refine, int transposed,
                                   DevProgState *states, int step, int rows_per_band, int n_split = 0, DevProgSub *subs = nullptr, int parts = 1);
// The first AC scans of large progressive batches, cut into chunks (progressive_chunks.hip): one restart segment of such a scan
struct DevAcSeg {
    int32_t image;                // the image (status, geometry)
    int32_t comp;                 // the scan's component
    int32_t ss, se, al;
    int32_t table;                // index of the scan's AC table in the batch
    int32_t stream_slot;          // the segment's number in stage 0's stream buffer (seg_bits index)
    int32_t stream_dw;            // its first dword there: (begin >> 2) + stream_slot
    int32_t first_blk, n_blk;     // blocks of the scan (its own raster): the segment's first, how many
    int32_t mcu_count_h;          // blocks per row of the scan
    int32_t last;                 // the scan's last restart segment
    int32_t chunk0, n_chunks;     // its chunks in the (padded) chunk list
};
constexpr int kProgCanonBytes = 320;     // per table behind its 9-bit LUT (512 x uint16: len << 8 | symbol): uint16 limit[16], int16 base[16], uint8 vals[256]
hipError_t launch_progressive_chunks(hipStream_t stream, const uint32_t *dstream, const int32_t *seg_bits, const DevAcSeg *segs, int n_segs,
                                     const uint8_t *tabs, const uint16_t *lut11p, const DevChunk *chunks, int64_t n_chunks, int cbits, uint64_t *exit_state,
                                     DevChunkOut *outs, void *items, int32_t *n_items, int32_t *owner, DevVSeg *vsegs, const DevImage *images,
                                     int16_t *coef, int32_t *status, int transposed, int max_links);
hipError_t launch_progressive_scan(hipStream_t stream, const uint8_t *blob, const DevProgSeg *segs, int n_segs,
                                   const DevProgScan *scans, const DevImage *images, const DevHuff *huff,
                                   int16_t *coef, int32_t *status, int spec_refine, int transposed, DevProgState *states,
                                   int step, int rows_per_band);
}

// stage-1 / stage-2 launchers (defined in huffman.hip / reconstruct.hip)
namespace mj {
hipError_t launch_huffman(hipStream_t stream, const uint8_t *blob, const DevSegment *segs, int64_t n_segs,
                          const DevImage *images, const DevHuff *huff, int16_t *coef, int32_t *status,
                          int lut_slots, int transposed);

#ifdef MJ_DIAGNOSTIC
void dbg_lanes_report();     // huffman_lanes.hip: prints and clears the in-loop stamps of MJ_DEBUG_STAGE1=3
void dbg_prog_report();      // progressive_fast.hip: ... of the refining walk
void dbg_prog_waves_report();       // progressive_fast.hip: when the waves of band launch MJ_DEBUG_PROG_STEP finished
void dbg_lanes13_waves_report();   // huffman_lanes13.hip: when every wave of the last launch finished
void dbg_fused_clear(uint8_t *dump);                   // fused.hip (MJ_DEBUG_FUSED): per-workgroup time stamps of the next launch ...
void dbg_fused_report(const uint8_t *dump, int n_wg);  // ... and their averages
#endif
// lane-parallel form: one restart segment per lane, all of the batch's tables (<= kMaxLaneTables) in LDS
constexpr int kLaneLutBits = 11;
constexpr int kMaxLaneTables = 8;
// per-workgroup table lists (batches with more tables than that): entries per workgroup; 8 or 16 of them are used
constexpr int kMaxWgTables = 16;
// what the launches of the lane family share (api.hip fills one per execute: lane_args)
struct LaneArgs {
    hipStream_t stream;
    const uint32_t *dstream; const int32_t *seg_bits;     // stage 0's output
    const DevSegment *segs; int64_t n_segs;               // restart segments (the lane launches of the synchronisation form: virtual segments)
    const DevImage *images;
    const DevHuff *huff;          // the batch's n_huff tables: code books, and
    const uint16_t *lut11;        // (len << 8 | symbol) for tables used as DC tables, (len << 11 | run << 4 | size, EOB = run 64) for AC tables
    int n_huff;
    int16_t *coef; int32_t *status; int transposed;
};
// the resolved AC tables and how the batch's tables map onto LDS slots: byte t of ac_slot_pk / dc_slot_pk = LDS slot of table t in
// that role, byte s of dc_tab_pk = table of DC slot s
struct ResolvedTables {
    const uint32_t *lut13;        // [n_ac][kLanes13SlotBytes / 4]: 8192 finished symbols + second-level tables for codes of 14..16 bits
    int n_ac, n_dc;
    uint64_t ac_slot_pk, dc_slot_pk, dc_tab_pk;
};
// stage 0 (destuff.hip): per restart segment, the bytes the bit reader keeps, as big-endian dwords at dword
// (begin >> 2) + segment index of `out_stream`; seg_bits[i] = 8 x kept bytes
hipError_t launch_destuff(hipStream_t stream, const uint8_t *blob, const DevSegment *segs, int64_t n_segs,
                          uint32_t *out_stream, int32_t *seg_bits);
hipError_t launch_scan_markers(hipStream_t stream, const uint8_t *blob, const DevScanJob *jobs, int n_jobs, DevSegment *segs,
                               int32_t *status);
// one counting round: entry == nullptr -> speculative round (every chunk assumes a block starts at its first bit);
// otherwise chunk c starts from entry[c - 1].  *changed counts the chunks whose exit state differs from prev_exit[c].
hipError_t launch_sync_count(const LaneArgs &a, const uint16_t *lut11u, const DevChunk *chunks, int64_t n_chunks, int cbits, const uint64_t *entry,
                             uint64_t *exit_out, DevChunkOut *outs, int32_t *changed, const int32_t *wg_tabs = nullptr, int wg_slots = 0,
                             const int32_t *prev_changed = nullptr, int warm_bits = -1);   // wg_tabs: per 256 chunks; warm_bits: run-up in front of every chunk, -1 = half a chunk
// the same on resolved tables (lutc: a.n_huff tables of tab_bytes each, wbits index bits: plan_create.hip's build_count_tables): the first
// walk over every chunk, then — max_links > 0 — the list of chunks whose entry state was guessed wrong (items: 16 bytes per
// chunk, *n_items) and their repair, each lane walking on for at most max_links chunks (owner: 4 bytes per chunk of scratch).
// exit_state / outs as above.
hipError_t launch_count(const LaneArgs &a, const uint32_t *lutc, int tab_bytes, int wbits, const DevChunk *chunks, int64_t n_chunks, int cbits,
                        int warm_bits, uint64_t *exit_state, DevChunkOut *outs, void *items, int32_t *n_items, int max_links, int32_t *owner);
// seg_chunk0[s] = the first chunk of restart segment s (a.n_segs + 1 entries)
hipError_t launch_build_vsegs(const LaneArgs &a, const DevChunk *chunks, const int32_t *seg_chunk0, const DevChunkOut *outs, DevVSeg *vsegs,
                              const uint64_t *final_exit, int cbits);
hipError_t launch_destuff_pieces(hipStream_t stream, const uint8_t *blob, const DevSegment *segs, const DevPiece *pieces,
                                 int64_t n_pieces, int32_t *kept, uint32_t *out_stream, int32_t *seg_bits);
hipError_t launch_huffman_lanes(const LaneArgs &a, const DevVSeg *vsegs = nullptr, const int32_t *wg_tabs = nullptr, int wg_slots = 0);   // wg_tabs: [workgroups][kMaxWgTables]
// the same with resolved 13-bit AC tables (huffman_lanes13.hip); a.lut11 supplies the DC tables
constexpr int kLanes13SubTables = 144;                              // second-level tables per AC table (8 entries each)
constexpr int kLanes13SlotBytes = 8192 * 4 + kLanes13SubTables * 32;  // one AC table in that form
bool lanes13_fits(int n_ac, int n_dc);
hipError_t launch_huffman_lanes13(const LaneArgs &a, const ResolvedTables &t, const DevVSeg *vsegs, const int32_t *by_length = nullptr,
                                  int order_mode = 0);   // by_length: segment numbers, longest first
// how that launch groups its units of work: lanes per wavefront (a workgroup = 4 waves = 4 x this many consecutive units)
int lanes_per_wave(int64_t n_segs, int n_slots);

// Test and tuning switches (mj_set_option, include/mijpeg.h): process-wide, set through the API only — the product library does
// not look at the environment for them (a stray variable must not change how a production decode runs); the diagnostic build
// (make DIAG=1) falls back to an environment variable of the same name so that the probe scripts can flip them per run.
// Returns the value or nullptr.
const char *opt(const char *name);
int set_opt(const char *name, const char *value);
int get_opt(const char *name, char *out, int cap);

constexpr size_t kStage2DumpBytes = 4096 * 1024;    // 1 KiB per workgroup of the largest persistent grid
// (MI355X: at most 768 workgroups use their KiB; two small areas further up have other uses)
constexpr size_t kDumpZeroLine = 0x180000;          // 16 bytes that stay zero (variant builds -DMJ_X_SPARSE_LD read them)
constexpr size_t kDumpClockWords = 0x1C0000;        // 4 x u64: shader-clock / 100 MHz stamps of the latest fused launch's workgroup 0 (mj_context_launch_clock)
struct ReconArgs {
    const DevImage *images;
    int32_t n_images;
    const int64_t *mcu_prefix;   // [n_images + 1]
    int64_t total_mcus;
    const int16_t *coef;
    const uint16_t *qt;          // [n_qt][64] natural order [v][u] (same layout as the coefficient blocks;
                                 // [u][v] like them when the plan is transposed)
    const double *idct_tt;       // [64 (u*8+v)][64 (x*8+y)] transposed reference table
    const uint32_t *up_taps;     // packed upsample taps, see reconstruct.hip
    uint8_t *rgb;
    uint8_t *dump;               // kStage2DumpBytes of writable memory: where stage 2's store instructions send the 16-byte
                                 // pieces that must not land in the image (lanes past an edge, strips that take the
                                 // slow stores) — the store phase stays branch-free, see reconstruct_fast.hip
    int16_t *planes;             // optional
    int16_t *idct_out;           // optional
    int32_t layout;
    int32_t exact_only;
    int32_t debug;               // diagnostic builds only (make DIAG=1, MJ_DEBUG_STAGE2 env): 1 = no IDCT rounds, 2 = no
                                 // pixel phase, 3 = no stores, 4 = in-kernel clock probe
    int32_t debug_mask;          // diagnostic builds only (MJ_DEBUG_MASK): ablations that combine — 1 no IDCT rounds (strip zeroed once),
                                 // 2 no pixel arithmetic, 4 no staging / stores, 8 stores to the dump line, 16 no level 2, 32 no coefficient loads
    // homogeneous-batch shortcut: all images share one geometry
    int32_t uniform_geometry;
    int32_t mcus_per_image;
    // fast form: the launch's strips are handed out in jobs of at most `chunk_strips` strips of one MCU column, one wavefront at
    // a time, through this ticket counter (zero before the launch; the wave that draws the launch's last ticket puts it back to zero)
    uint32_t *work_counter;
    int32_t chunk_strips;
    int32_t jobs_per_ticket;     // >= 1
    unsigned long long *level_counts;   // seam-output launches: blocks seen / sent to level 2 / sent to level 3 (mj_plan_idct_levels), per plan
    // window plans (mj_plan_request.rois): per image, the window stage 2 writes (null: whole images).  The exact-order and generic
    // kernels then number the windows' MCUs only: total_mcus and mcu_prefix count those, uniform_geometry is 0.
    const DevWindow *win;
};
hipError_t launch_reconstruct(hipStream_t stream, const ReconArgs &a, int hmax, int vmax, int ncomp);
// any sampling factors 1..4 per component (DevImage::generic): reconstruct.hip
hipError_t launch_reconstruct_generic(hipStream_t stream, const ReconArgs &a);
// fast form: strips of fast_tile_mcus() MCUs in column-major MCU order.  transposed = the kernel runs on the transposed
// image (blocks and tables stored [u][v]), so its x-major output is the row-major image (MJ_LAYOUT_ROWMAJOR)
int fast_tile_mcus(int hmax, int vmax, int ncomp, bool transposed);
// how many times the 64 lanes' MCUs a strip is tall (FGeo::SV): MCUs of 8 pixel rows whose column runs would be under 192 bytes
constexpr int strip_sv(int mw, int mh, int nc) { return mh != 8 ? 1 : ((64 / mw) * 8 * nc >= 192 ? 1 : ((64 / mw) * 8 * nc == 64 ? 4 : 2)); }
// jobs: pieces of at most a.chunk_strips strips of one MCU column, numbered image by image (job_prefix[i] = first job of image i)
hipError_t launch_reconstruct_fast(hipStream_t stream, const ReconArgs &a, int hmax, int vmax, int ncomp, bool transposed,
                                   const int64_t *job_prefix, int64_t total_jobs, int jobs_per_image);
// Stages 1 + 2 in one launch (fused.hip): producer wavefronts (the lane walk) and consumer wavefronts (stage 2's strip worker)
// in one workgroup per CU that takes whole images — `ipw` of them at a time, in `n_pass` passes when a workgroup's images hold
// more restart segments than its producers have lanes (8 x 64).  fused_shape() says how such a launch would be cut — ok =
// false: it does not apply (LDS) and the two launches stay.
constexpr int kFusedPassShift = 20;     // a producer's progress word: pass << 20 | MCUs of its segments complete in that pass
struct FusedShape {
    bool ok;
    int ipw;            // images per workgroup and pass
    int n_pass;         // passes of a workgroup: its "virtual workgroups" n_pass * wg + pass, one after the other
    int n_virt;         // virtual workgroups in all = ceil(images / ipw)
    int n_prod, lpw;    // producer wavefronts, lanes (restart segments) per producer wavefront
    int n_cons;         // consumer wavefronts beside the producers (every wavefront is one once the producers are through)
    int ring;           // bytes of stream window per lane
    int ac_total_bytes; // the AC tables in LDS, back to back (12-bit main levels — 13 where the plan says so — + their second-level tables)
    int dbits;          // index bits of the DC tables in LDS
    bool xwg;           // restart segments dealt out by length: one pool of jobs for the launch, hand-off across workgroups
    int n_wg;           // ... workgroups of such a launch (= CUs: all resident at once)
};
FusedShape fused_shape_x(int cus, int ac_total_bytes, int n_dc, int hmax, int vmax, bool transposed, int64_t n_segs, int want_consumers);
FusedShape fused_shape(int cus, int ac_total_bytes, int n_dc, int hmax, int vmax, bool transposed, int n_images, int spi, int want_consumers,
                       int want_producers = 0);
// spi: restart segments per image; restart_interval: MCUs per segment (any: a job's readiness is worked out per MCU)
hipError_t launch_fused(const LaneArgs &l, const ResolvedTables &t, const FusedShape &shape, const int ac_off[4], const int ac_bits[4],
                        const ReconArgs &a, int hmax, int vmax, int spi, int restart_interval, int mcus_per_row, int mcu_rows,
                        const int64_t *job_prefix, int64_t total_jobs, int jobs_per_image, const int32_t *by_length = nullptr,
                        const int32_t *holder = nullptr, uint32_t *x_words = nullptr);
// (t.lut13 of launch_fused: the plan's fused tables, back to back — ac_off / ac_bits per LDS slot)
// Launch-geometry caches are per device: one process may hold contexts on several GPUs (mijpeg.h: one context per GPU per
// thread), and a function attribute set on one device says nothing about the next.  Contexts on two threads may make a
// kernel's FIRST launch at the same moment: the per-device flags are std::once_flag (OncePerDevice), the cached integers atomics.
constexpr int kMaxDevices = 64;
inline int current_device() { int d = 0; (void)hipGetDevice(&d); return d >= 0 && d < kMaxDevices ? d : 0; }
struct OncePerDevice {
    std::once_flag flag[kMaxDevices];
    template <class F> void run(F &&fn) { std::call_once(flag[current_device()], fn); }
};
struct IntPerDevice {         // 0 = not known yet; racing first uses compute and store the same value
    std::atomic<int> v[kMaxDevices];
    IntPerDevice() { for (auto &x : v) x.store(0, std::memory_order_relaxed); }
    template <class F> int get(F &&compute) {
        std::atomic<int> &x = v[current_device()];
        int r = x.load(std::memory_order_relaxed);
        if (r == 0) { r = compute(); x.store(r, std::memory_order_relaxed); }
        return r;
    }
};
inline int device_cus() {
    static IntPerDevice cus;
    return cus.get([] {
        int c = 0;
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, current_device()) != hipSuccess || c < 1) c = 256;
        return c;
    });
}
// MJ_LAYOUT_PLANAR_*: every image's interleaved pixels (x-major or row-major, as stage 2 wrote them) -> its three planes
// (win: window plans — every image's window instead of the image)
hipError_t launch_planes_from_interleaved(hipStream_t stream, const DevImage *images, int n_images, int64_t max_pixels,
                                          const uint8_t *interleaved, uint8_t *planar, const DevWindow *win = nullptr);
// window plans of MJ_FLAG_GPU_SEGMENT batches: out[i] = full[idx[i]] — the restart segments the windows need, out of the
// list the marker scan filled, into the list stages 0 and 1 read
hipError_t launch_gather_segments(hipStream_t stream, const DevSegment *full, const int32_t *idx, int64_t n, DevSegment *out);
// ---- resize.hip: decode to a fixed size (plan creation: resize_plan.hip)
// One image of a resized plan: where its decoded pixels (the image, or its window) lie in the plan's intermediate buffer,
// their size, its tap tables and where its out_width x out_height pixels go.
struct DevResizeImage {
    int64_t src_off;      // bytes, into the intermediate buffer (= DevImage::rgb_off)
    int64_t dst_off;      // bytes, into the output: slot * out_width * out_height * ncomp
    int32_t w, h;         // size of the source pixels
    int32_t xtab, ytab;   // word offsets of its width / height tables in ResizeArgs::tabs
};
// (a table: ksize, first source index [out], tap count [out], taps [out][ksize])
struct ResizeArgs {
    const uint8_t *src;
    uint8_t *dst;
    const DevResizeImage *images;
    const int32_t *tabs;
    int32_t n_images, ow, oh, layout;
    int32_t tr, tc, tiles_x, tiles_y;         // output rows / columns per tile, tiles per image
    int32_t t_pitch, tab_off, stage_off, stage_bytes, lds_bytes;    // the workgroup's LDS (resize.hip)
    // the output element (mj_plan_request.output): esize 1 stores the resized byte itself; 2 / 4 store lut[c * 256 + byte],
    // the byte's float16 / bfloat16 / float32 bit pattern, which every workgroup first copies to lut_off of its LDS
    // mirror: NULL, or one byte per image, != 0: that image is stored flipped along the width axis, column out_width - 1 - x
    // (an array of its own, read by the mirror instances only: the image record keeps its 32 bytes, and with them the plain
    // instances the code they were)
    const void *lut;
    const uint8_t *mirror;
    int32_t esize, lut_off;
    // oriented plans (mj_plan_request.orientations with a size): 0 = none.  1: `mirror` holds, per image, bit 0 = store at column
    // out_width - 1 - x, bit 1 = store at row out_height - 1 - y (the image's tap tables are the reversed ones, so the sums are
    // those of the flipped source; a mirror flag is folded into bit 0).  2: the same, and the images are transposing
    // orientations: the source is read as the other layout's kernel reads it (the stored rows are the oriented columns)
    int32_t orient;
    // 1: a filter whose taps go below zero (bicubic, Lanczos) — the signed instances; a mirror flag then travels as an
    // oriented plan's bit 0 does (launch_resize)
    int32_t sgn;
};
constexpr int64_t kResizeGridX = 1 << 20;      // workgroups along x of the resize launch's grid (the rest along y)
// (filter: MJ_FILTER_*, one that resize_filter_known)
bool resize_filter_known(int filter);
bool resize_filter_signed(int filter);
// (box: NULL — the whole axis, [0, in_size) — or the part {in0, in1} of it the table resamples, as 32-bit floats: Pillow's
// precompute_coeffs(inSize, in0, in1, outSize), the resample behind a reduce, reduce.hip)
int resize_axis_ksize(int in_size, int out_size, int filter = 0, const float *box = nullptr);
void build_resize_axis(int in_size, int out_size, int32_t *xmin, int32_t *count, int32_t *taps, int taps_stride, int filter = 0, const float *box = nullptr);
// (out_ncomp: 0 or ncomp — the instances there were; else a plan that converts, mj_plan_request.mode with a size)
// (placed: a plan of mj_plan_request.places — the placed instances, which store `fill`, byte c in bits 8c..8c+7, where
// the image does not cover the canvas; a.mirror is then set)
hipError_t launch_resize(hipStream_t stream, const ResizeArgs &a, int ncomp, int out_ncomp = 0, int placed = 0, unsigned fill = 0);
// ---- reduce.hip: the first step of a two-step resize (mj_plan_request.reducing_gap; tools/reduce_model.py)
// One image of a reducing plan, as rows x len pixels (len along the contiguous axis) of the plan's intermediate buffer: every
// cell of f_slow x f_fast pixels becomes one pixel of the reduced image, ((sum + n / 2) * m(n)) >> 24 with n the cell's own
// pixel count.  Cell k of an axis is [k * f - off, (k + 1) * f - off) clipped to the axis: off 0 puts the partial cell last,
// off = f - size mod f first (an axis the orientation reverses).  mul / half: m(n) and n / 2 for the four kinds of cell —
// bit 0: partial along the contiguous axis, bit 1: partial along the rows — evaluated on the host (reduce_multiplier).
struct DevReduceImage {
    int64_t src_off, dst_off;     // bytes: into the intermediate buffer, into the buffer of reduced images
    int32_t rows, len;
    int32_t f_slow, f_fast, off_slow, off_fast;
    uint32_t mul[4], half[4];
    int32_t pitch;                // pixels from one source row to the next: len, but for a view (mj_plan_request.views), whose rows
                                  // are rows of the decoded image it is a window of
};
struct ReduceArgs {
    const uint8_t *src;
    uint8_t *dst;
    const DevReduceImage *images;
    int32_t n_images;
    int32_t tile_slow, tile_fast;       // reduced rows / reduced pixels of a row per workgroup
    int32_t tiles_slow, tiles_fast;     // tiles per image: those of the largest reduced image (a smaller one's rest idles)
};
constexpr int kReduceStage = 4096;       // bytes of a source row a wavefront stages at a time
constexpr int kReduceMaxCell = 65536;    // pixels per cell: every sum stays below 2^24 and every product inside 32 bits
// Image.resize's factors for src -> dst with reducing_gap `gap` (doubles, divided in this order)
void reduce_factors(int src_w, int src_h, int dst_w, int dst_h, double gap, int *fx, int *fy);
uint32_t reduce_multiplier(uint32_t n);      // (uint32)(float32(2^32) / float32(256 n))
// the record of one image but for its offsets (phases: size mod f where the axis is reversed, else 0); pitch = len
void reduce_record(int rows, int len, int f_slow, int f_fast, int phase_slow, int phase_fast, DevReduceImage *out);
// the kernel's arithmetic on the host: ncomp interleaved components; luma: three components in, mode_luma of each pixel summed, one out
void reduce_host(const uint8_t *src, const DevReduceImage &im, int ncomp, bool luma, uint8_t *out);
// (luma: the instance that converts colour to L where it reads, mj_plan_request.mode with MJ_MODE_L)
hipError_t launch_reduce(hipStream_t stream, const ReduceArgs &a, int ncomp, bool luma);
int reduce_tile_fast(int out_ncomp);     // reduced pixels of a row a workgroup takes
int reduce_piece(int src_ncomp);         // source pixels of a row a wavefront stages at a time (the instance's kPiece)
// ---- affine.hip: the affine transform in front of the window and the resize (mj_plan_request.affine; tools/affine_model.py)
// One output of a plan with an affine transform: the stored image it is made of (sw x sh pixels of the plan's intermediate
// buffer, in the plan's layout), the oriented image's size w x h — what Pillow's rules count in —, the window of the transformed
// image that is written (densely, win_w x win_h, in the plan's layout, at dst_off of the second buffer), and the rule:
//   kind 0  no transform: the oriented pixels of the window
//        1  NEAREST by tables: xtab / ytab (word offsets into AffineArgs::tabs) hold the source column / row of every column / row
//           of the window, -1: outside
//        2  NEAREST in 16.16 fixed point: fx[6]
//        3  BILINEAR, 4 BICUBIC: a[6] in doubles
struct DevAffineImage {
    int64_t src_off, dst_off;
    int32_t sw, sh, w, h;
    int32_t x0, y0, win_w, win_h;
    int32_t kind, obits;          // obits: orient_bits of the image's orientation
    int32_t xtab, ytab;
    int32_t fx[6];
    double a[6];
};
struct AffineArgs {
    const uint8_t *src;
    uint8_t *dst;
    const DevAffineImage *images;
    const int32_t *tabs;
    int32_t n_images, layout;           // layout & 1: row-major
    int32_t tiles_slow, tiles_fast;     // tiles per output: those of the largest window (a smaller one's rest idles)
    uint32_t fill;                      // byte c in bits 8c..8c+7, per OUTPUT component
};
constexpr int kAffineTileFast = 64, kAffineTileSlow = 16;      // pixels of a tile along the layout's contiguous axis / across it
// what mj_plan_request.affine and mj_host_affine refuse of one matrix for a w x h image: nullptr, or the reason
const char *affine_fault(const double *a, int filter, int w, int h);
// the rule's kind for a matrix (filter: MJ_AFFINE_*), its fixed-point form, and the index table of one axis of the NEAREST scale
// path: entry j is the source index of output index first + j, accumulated from index 0 as Pillow does (-1: outside [0, size))
int affine_kind(const double *a, int filter);
void affine_fixed(const double *a, int32_t fx[6]);
void affine_scale_table(double scale, double offset, int size, int first, int n, int32_t *out);
// the kernel's arithmetic on the host, for an upright row-major image (obits 0, layout 1); tabs as AffineArgs::tabs
void affine_host(const uint8_t *src, const DevAffineImage &im, const int32_t *tabs, int ncomp, int out_ncomp, uint32_t fill, uint8_t *out);
// (ncomp: the decoded images'; out_ncomp: the written ones' — the same, 1 for colour to L, 3 for grey to RGB)
hipError_t launch_affine(hipStream_t stream, const AffineArgs &a, int ncomp, int out_ncomp);
// ---- affine.hip: the perspective transform in the same place (mj_plan_request.perspective;
// tools/perspective_model.py).  One output of such a plan: DevAffineImage's image, window and orientation, and the rule:
//   kind 0  no transform: the oriented pixels of the window
//        1  NEAREST: the truncated coordinates, in doubles
//        3  BILINEAR, 4 BICUBIC (DevAffineImage's numbers: the taps are the same code)
// with c[8] for all three: no tables, no fixed point.  The launch's geometry is the affine launch's (kAffineTile*).
struct DevPerspectiveImage {
    int64_t src_off, dst_off;
    int32_t sw, sh, w, h;
    int32_t x0, y0, win_w, win_h;
    int32_t kind, obits;
    double c[8];
};
struct PerspectiveArgs {
    const uint8_t *src;
    uint8_t *dst;
    const DevPerspectiveImage *images;
    int32_t n_images, layout;
    int32_t tiles_slow, tiles_fast;
    uint32_t fill;
};
// what the field and mj_host_perspective refuse of one set of coefficients for a w x h image (no magnitude is refused: the rule
// has no fixed point, and a coordinate of any size, NaN included, is tested before it is used): nullptr, or the reason
const char *perspective_fault(const double *c, int filter, int w, int h);
int perspective_kind(int filter);
void perspective_host(const uint8_t *src, const DevPerspectiveImage &im, int ncomp, int out_ncomp, uint32_t fill, uint8_t *out);
hipError_t launch_perspective(hipStream_t stream, const PerspectiveArgs &a, int ncomp, int out_ncomp);
// ---- colour.hip: colour operations on the finished canvas (mj_plan_request.colour; tools/colour_model.py)
// One output of a plan with colour operations: its chain (n ops; value: the factor of brightness, color, contrast and sharpness;
// ivalue: posterize's MASK and solarize's clamped threshold, as integers — colour_ivalue; a blur's r, with ww and fw beside it —
// colour_blur_pass; adjust_hue's shift, the only thing the launches see of its factor), where its elements go in the caller's array (dst_off, in ELEMENTS) and whether it is mirrored.
struct DevColourOutput {
    int64_t dst_off;
    int32_t n, mirror;
    int32_t kind[4];
    float value[4];
    int32_t ivalue[4];
};
// The canvases are n_outputs images of ow x oh pixels of C components in the plan's layout, output after output.  A pixel's
// place is p = y * ow + x (row-major layouts) or x * oh + y (x-major); component c of it is byte p * C + c (interleaved) or
// c * ow * oh + p (planar) of its image.  hist: uint32[n_outputs][4][256] — components 0..2 and L —, tables: uint8[n_outputs][3][256].
// hist_list[hist_first[s] .. hist_first[s + 1]): the outputs whose op s takes a histogram; tables_at bit s: some output's op s is a table
struct ColourArgs {
    uint8_t *canvas[2];
    uint32_t *hist;
    uint8_t *tables;
    const DevColourOutput *outputs;
    const int32_t *hist_list;
    const void *lut;                    // the output table (ResizeArgs::lut's), NULL for bytes
    void *dst;
    int32_t hist_first[5];
    int32_t n_outputs, ow, oh, C, layout, esize, steps, tables_at;
};
// What the blur launches take beside ColourArgs (which the other launches take as it was).  list[first[s] .. first[s + 1]): the
// outputs whose op s is a blur (the plan's list array, behind the histogram lists); passes[s]: the passes of step s's longest
// blur (6: some Gaussian, 2: boxes only, 0: no blur).  lds: the bytes of LDS a workgroup of the plane-resident launch takes — two
// planes of oh rows of ow bytes rounded up to whole dwords —, or 0 on a plan that blurs pass by pass through `scratch`, a third
// canvas (kBlurLdsMax; option MJ_BLUR)
struct ColourBlurArgs {
    const int32_t *list;
    const uint32_t *weights;            // [n_outputs][4 steps][2]: ww and fw of output k's op s where that is a blur (the record keeps its size)
    uint8_t *scratch;
    int32_t first[5];
    int32_t passes[4];
    int32_t lds;
};
// What the hue launch takes beside ColourArgs.  list[first[s] .. first[s + 1]): the outputs of three components whose op s is
// adjust_hue (the plan's list array, behind the blur lists); tables: the plan's copy of colour_hue_tables()
struct HueTables;
struct ColourHueArgs {
    const int32_t *list;
    const HueTables *tables;
    int32_t first[5];
};
constexpr int kColourHistPixels = 4096;       // pixels of a canvas one workgroup of the histogram launch counts
constexpr int kBlurLdsMax = 160 * 1024;       // the LDS of a gfx950 workgroup: what two planes of a canvas must fit in
constexpr float kBlurMaxRadius = 1024.0f;
inline int64_t blur_lds_bytes(int ow, int oh) { return 2 * (int64_t)((ow + 3) & ~3) * oh; }
// Image.blend of one byte (tools/colour_model.py: blend); every operation rounds on its own (-ffp-contract=off, host and device)
__host__ __device__ inline unsigned colour_blend(int d, int v, float alpha) {
    const float t = (float)d + alpha * (float)(v - d);
    if (alpha >= 0.0f && alpha <= 1.0f) return (unsigned)t;
    return t <= 0.0f ? 0u : t >= 255.0f ? 255u : (unsigned)t;
}
// ImageFilter.SMOOTH of one interior pixel from its 3 x 3 neighbourhood p[row][column], row 0 above
__host__ __device__ inline unsigned colour_smooth(const float p[3][3]) {
    const float k1 = (float)(1 / 13.0), k5 = (float)(5 / 13.0);
    float ss = 0.5f;
    ss += (p[2][0] * k1 + p[2][1] * k1) + p[2][2] * k1;
    ss += (p[1][0] * k1 + p[1][1] * k5) + p[1][2] * k1;
    ss += (p[0][0] * k1 + p[0][1] * k1) + p[0][2] * k1;
    return ss <= 0.0f ? 0u : ss >= 255.0f ? 255u : (unsigned)ss;
}
// One pass of Pillow's box blur (BoxBlur.c; tools/colour_model.py: box_pass) at place x of a line of n bytes `stride` apart, in
// 32-bit unsigned arithmetic: blur_window is the sum of in[clamp(x + d)], d = -r .. r, as count_left * in[0] + the part inside
// the line + count_right * in[n - 1] — at most n terms, whatever r —, blur_byte the weighted sum's byte
__host__ __device__ inline uint32_t blur_byte(uint32_t ww, uint32_t fw, uint32_t sum, uint32_t far) { return ((ww * sum + fw * far + (1u << 23)) >> 24) & 0xFFu; }
__host__ __device__ inline uint32_t blur_window(const uint8_t *line, int64_t stride, int n, int x, int r) {
    const int lo = x - r > 0 ? x - r : 0, hi = x + r < n - 1 ? x + r : n - 1;
    uint32_t s = (uint32_t)(lo - (x - r)) * line[0] + (uint32_t)(x + r - hi) * line[(int64_t)(n - 1) * stride];
    for (int i = lo; i <= hi; ++i) s += line[(int64_t)i * stride];
    return s;
}
__host__ __device__ inline uint32_t blur_pixel(const uint8_t *line, int64_t stride, int n, int x, int r, uint32_t ww, uint32_t fw) {
    const int a = x - r - 1 > 0 ? x - r - 1 : 0, b = x + r + 1 < n - 1 ? x + r + 1 : n - 1;
    return blur_byte(ww, fw, blur_window(line, stride, n, x, r), (uint32_t)line[(int64_t)a * stride] + line[(int64_t)b * stride]);
}
__host__ __device__ inline bool colour_is_blur(int kind) { return kind == MJ_COLOUR_GAUSSIAN_BLUR || kind == MJ_COLOUR_BOX_BLUR; }
// passes along each axis
__host__ __device__ inline int colour_blur_passes(int kind) { return kind == MJ_COLOUR_GAUSSIAN_BLUR ? 3 : 1; }
// whether an output of C components whose op is `kind` is another launch's than k_colour_apply's: a blur, or adjust_hue on three
// components (on one component adjust_hue is the identity: k_colour_apply's copy)
__host__ __device__ inline bool colour_is_elsewhere(int kind, int C) { return colour_is_blur(kind) || (kind == MJ_COLOUR_ADJUST_HUE && C == 3); }
// whether an op is a look-up table per component / takes a histogram
__host__ __device__ inline bool colour_is_table(int kind) {
    return kind != MJ_COLOUR_COLOR && kind != MJ_COLOUR_SHARPNESS && kind != 0 && !colour_is_blur(kind) && kind != MJ_COLOUR_ADJUST_HUE;
}
__host__ __device__ inline bool colour_needs_hist(int kind) { return kind == MJ_COLOUR_CONTRAST || kind == MJ_COLOUR_AUTOCONTRAST || kind == MJ_COLOUR_EQUALIZE; }
// Entry i of a table-shaped op's table for one component.  st: that component's histogram, scanned (ops that take one) — lo, hi
// its first and last non-empty bins, nz how many are non-empty, last the last one's count, total the sum of all —, with mean
// contrast's grey level, which comes from the L histogram; prefix: the sum of the component's bins below i (equalize)
struct ColourStats { int lo, hi, nz, mean; unsigned long long last, total; };
__host__ __device__ inline unsigned colour_table_entry(int kind, float value, int ivalue, int i, const ColourStats &st, unsigned long long prefix) {
    switch (kind) {
    case MJ_COLOUR_BRIGHTNESS: return colour_blend(0, i, value);
    case MJ_COLOUR_CONTRAST: return colour_blend(st.mean, i, value);
    case MJ_COLOUR_POSTERIZE: return (unsigned)i & (unsigned)ivalue;
    case MJ_COLOUR_SOLARIZE: return i < ivalue ? (unsigned)i : 255u - (unsigned)i;
    case MJ_COLOUR_INVERT: return 255u - (unsigned)i;
    case MJ_COLOUR_AUTOCONTRAST: {
        if (st.hi <= st.lo) return (unsigned)i;
        const double scale = 255.0 / (double)(st.hi - st.lo), offset = (double)(-st.lo) * scale;
        const double t = (double)i * scale + offset;
        return t <= 0.0 ? 0u : t >= 255.0 ? 255u : (unsigned)(int)t;
    }
    case MJ_COLOUR_EQUALIZE: {
        if (st.nz <= 1) return (unsigned)i;
        const unsigned long long step = (st.total - st.last) / 255u;
        if (!step) return (unsigned)i;
        const unsigned long long q = (step / 2 + prefix) / step;
        return q > 255u ? 255u : (unsigned)q;
    }
    }
    return (unsigned)i;
}
// adjust_hue (MJ_COLOUR_ADJUST_HUE; tools/colour_model.py: rgb_to_hsv, hsv_to_rgb): Pillow's Convert.c both ways around H + shift.
// What the second conversion makes of one byte alone is tabled — by the H byte: hf = (float)H * 6.0 / 255.0 in double, its floor's
// i % 6 (sextant) and f = (float)(hf - i); by the S byte: fs = (float)(S / 255.0) —, which takes every division out of it
struct HueTables { float f[256]; float fs[256]; uint8_t sextant[256]; };
inline HueTables colour_hue_tables() {
    HueTables t;
    for (int b = 0; b < 256; ++b) {
        const double hf = (double)(float)b * 6.0 / 255.0, i = floor(hf);
        t.f[b] = (float)(hf - i); t.sextant[b] = (uint8_t)((int)i % 6);
        t.fs[b] = (float)((double)b / 255.0);
    }
    return t;
}
// rgb2hsv_row of one pixel.  Of rc, gc, bc = (float)(max - component) / cr only the two the branch takes are divided: h = base + a - b
// in double with base 0 (r is the max: bc - gc, which a float subtraction rounds alike), 2 (g: rc - bc) or 4 (gc - rc).  h / 6 + 1
// lies in [5 / 6, 11 / 6], where fmod(., 1.0) is the subtraction of 1 from what is not below it, and exact
__host__ __device__ inline void colour_rgb_to_hsv(unsigned r, unsigned g, unsigned b, unsigned &H, unsigned &S, unsigned &V) {
    const unsigned maxc = r > g ? (r > b ? r : b) : (g > b ? g : b), minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    V = maxc; H = S = 0;
    if (maxc == minc) return;
    const float cr = (float)(int)(maxc - minc), s = cr / (float)(int)maxc;
    const unsigned na = r == maxc ? maxc - b : g == maxc ? maxc - r : maxc - g, nb = r == maxc ? maxc - g : g == maxc ? maxc - b : maxc - r;
    const double base = r == maxc ? 0.0 : g == maxc ? 2.0 : 4.0;
    const float fa = (float)(int)na / cr, fb = (float)(int)nb / cr;
    const float h = (float)((base + (double)fa) - (double)fb);
    double w = (double)h / 6.0 + 1.0;
    if (w >= 1.0) w -= 1.0;
    const int ih = (int)((double)(float)w * 255.0), is = (int)((double)s * 255.0);
    H = (unsigned)(ih > 255 ? 255 : ih); S = (unsigned)(is > 255 ? 255 : is);
}
// C's round of a double in 0 .. 255 (x - trunc(x) is exact)
__host__ __device__ inline unsigned colour_hue_round(double x) {
    const double t = trunc(x);
    return (unsigned)(int)(x - t >= 0.5 ? t + 1.0 : t);
}
// hsv2rgb of one pixel, the tables' three entries given.  p = round(V * (1.0 - fs)); an odd sextant takes q = round(V * (1.0 - fs * f))
// — a float product —, an even one t = round(V * (1.0 - fs * (1.0 - f))) — in double —: u is the one of them this sextant has
__host__ __device__ inline void colour_hsv_to_rgb(unsigned S, unsigned V, int sextant, float f, float fs, unsigned *rgb) {
    rgb[0] = rgb[1] = rgb[2] = V;
    if (S == 0) return;
    const double v = (double)(int)V, dfs = (double)fs;
    const unsigned p = colour_hue_round(v * (1.0 - dfs));
    const unsigned u = colour_hue_round(v * (1.0 - (sextant & 1 ? (double)(fs * f) : dfs * (1.0 - (double)f))));
    switch (sextant) {
    case 0: rgb[1] = u; rgb[2] = p; break;
    case 1: rgb[0] = u; rgb[2] = p; break;
    case 2: rgb[0] = p; rgb[2] = u; break;
    case 3: rgb[0] = p; rgb[1] = u; break;
    case 4: rgb[0] = u; rgb[1] = p; break;
    default: rgb[1] = p; rgb[2] = u; break;
    }
}
// adjust_hue of one pixel: to HSV, H + shift mod 256, and back (tf, tfs, tsext: HueTables' arrays, wherever they lie)
__host__ __device__ inline void colour_hue(unsigned r, unsigned g, unsigned b, int shift, const float *tf, const float *tfs, const uint8_t *tsext, unsigned *rgb) {
    unsigned H, S, V;
    colour_rgb_to_hsv(r, g, b, H, S, V);
    H = (H + (unsigned)shift) & 255u;
    colour_hsv_to_rgb(S, V, tsext[H], tf[H], tfs[S], rgb);
}
// what mj_plan_request.colour and mj_host_colour_ops refuse of one chain: nullptr, or the reason
const char *colour_fault(const mj_colour_chain &c);
// the integer form of an op's value (posterize: the mask, solarize: the clamped threshold, a blur: r, adjust_hue: the shift; else 0)
int colour_ivalue(const mj_colour_op &op);
// a blur's pass: r, ww and fw of its box radius (gaussian_blur: the radius of the box whose three passes stand for it)
struct BlurPass { int32_t r; uint32_t ww, fw; };
BlurPass colour_blur_pass(const mj_colour_op &op);
// the launches of one execute: the canvas in a.canvas[0] -> a.dst
hipError_t launch_colour(hipStream_t stream, const ColourArgs &a, const ColourBlurArgs &b, const ColourHueArgs &h);
// ---- output colour mode (tools/mode_model.py)
// Pillow's convert("L") of one RGB pixel: (19595 R + 38470 G + 7471 B + 32768) >> 16 — at most 65536 * 255 + 32768, far inside 32 bits
__host__ __device__ inline unsigned mode_luma(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }
// a batch's component count is its first image's (1, else 3; 3 when there is no image to ask)
inline int batch_ncomp(const mj_batch *b) { return b && b->n_images > 0 && b->images && b->images[0].ncomp == 1 ? 1 : 3; }
// ---- orient.hip: EXIF orientation at the files' own sizes
// One image of an oriented plan: its stored-order pixels in the plan's intermediate buffer as rows x len pixels (len along
// the contiguous axis: row-major plans height x width, x-major plans width x height) and what becomes of them — op bit 0:
// the destination's rows run backwards, bit 1: its contiguous axis runs backwards, bit 2: rows and columns change places.
struct DevOrientImage {
    int64_t src_off, dst_off;     // bytes; an image keeps its place in the packing (orientation keeps the pixel count; a plan that
                                  // converts, mj_plan_request.mode, packs the same pixels with the output's components)
    int32_t rows, len;
    int32_t tiles_l;              // tiles along the contiguous axis
    int32_t op;
};
struct OrientArgs {
    const uint8_t *src;
    uint8_t *dst;
    const DevOrientImage *images;
    const int64_t *tile_prefix;   // [n_images + 1]: first tile of every image, then the total
    int64_t total_tiles;
    int32_t n_images, planar;     // planar: the destination holds the components one plane after the other
};
hipError_t launch_orient(hipStream_t stream, const OrientArgs &a, int ncomp, int out_ncomp = 0);      // (out_ncomp as launch_resize's)
// bits[v] = the bit pattern (in the low esize bytes) of resized byte v as an MJ_DTYPE_F16 / BF16 / F32 element:
// fl32(fl32(fl32(v) / 255 - mean) / std), then rounded to nearest even into the 16-bit types (tools/normalize_model.py)
void build_normalize_table(int dtype, float mean, float std, uint32_t *bits);
// dst[0 .. bytes) = src[0 .. bytes), sixteen bytes per lane (bytes a multiple of 16): the plain copy the rooflines are held against
hipError_t launch_copy16(hipStream_t stream, const void *src, void *dst, int64_t bytes, int variant);     // variant 0 .. copy16_variants() - 1: launch shapes
int copy16_variants();
// p[0 .. n_words) = value, as a kernel (why not hipMemsetAsync: api.hip)
hipError_t launch_fill_words(hipStream_t stream, void *p, uint32_t value, int64_t n_words);
// 64-entry permutation of every block: dst[b*64 + i] = src[b*64 + table[i]]
hipError_t launch_permute_blocks(hipStream_t stream, const int16_t *src, int16_t *dst, int64_t n_blocks, int to_natural,
                                 int transposed);
}  // namespace mj
