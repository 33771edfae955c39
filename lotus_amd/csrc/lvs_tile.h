// Launch interface of the tiled distance / top-k kernel (lvs_tile.hip) and the small-batch kernel (lvs_stream.hip).
#pragma once
#include "lvs_common.h"
#include "lvs_ivf_plan.h"  // the IVF scans' shapes (LVS_IVF_TILEQ, ...), LDS sizes and fits

#define LVS_MODE_TOPK 0
#define LVS_MODE_SCORES 1
#define LVS_MODE_TOP1 2
#define LVS_MODE_RANGE 3
#define LVS_MODE_COLLECT 4
#define LVS_MODE_TOP2 5     // TOP1 + the runner-up score per query (certified nearest-row search, lvs_nearest_hi)
#define LVS_MODE_SEED 6     // best TOPK-domain score of every (slab, query): seeds the thresholds of a launch with few query tiles

struct LvsTileArgs {
    const void* xb;           // [nb][ld] fp16 packed corpus shard
    const void* xq;           // [nq][ld] fp16 packed queries
    const float* bn;          // [nb] |y|^2 (L2 only)
    const float* qn;          // [nq] |q|^2 (L2 only)
    const uint32_t* row_ids;  // nullable [nb]: id reported for a shard row
    const u64* ub;            // nullable: per-query exclusive upper bound key (multi-pass k > LVS_KPASS)
    long long ub_stride;      // stride of ub in u64 elements
    uint32_t* gtau;           // [nq] shared running thresholds (ord32 of the k-th best score), zero-initialised
    u64* out;                 // [nslab][nq][k] per-slab candidate keys
    float* out_second;        // LVS_MODE_TOP2: [nslab][nq] runner-up score ("better" domain) of every slab
    float* seed_out;          // LVS_MODE_SEED: [nslab][nq] best score of every slab, bit-identical to the score LVS_MODE_TOPK ranks
    float* scores;            // LVS_MODE_SCORES: [nq][ld_scores]
    // LVS_MODE_RANGE: emit (query, corpus row, score) for score > threshold
    long long* pair_q;
    long long* pair_j;
    float* pair_s;
    unsigned long long* pair_count;
    long long pair_capacity;
    long long q_row0;         // >= 0: self-join, query r is corpus row q_row0 + r and only pairs j > i are kept
    long long q_base;         // RANGE: added to the query numbers written to pair_q (a launch over a slice of the call's queries)
    float threshold;
    float out_scale;          // SCORES / RANGE: factor applied to a score on its way out (2^-e of operands packed with a scale)
    int qt_stride, qt_phase;  // only query tiles with qt % qt_stride == qt_phase are processed (multi-GPU deal)
    long long ld_scores;
    long long nb, nq;
    long long ldb, ldq;       // leading dimensions in halfs (corpus / queries)
    long long id_offset;
    int nkd;                  // padded d / 64
    int nk;                   // K-steps per tile = nseg * nkd
    int nseg;                 // K segments: product = sum over segments of q[seg_q..] . y[seg_c..]
    int seg_q[3], seg_c[3];   // column offsets (halfs) of each segment in the query / corpus rows
    int metric;
    int k;                    // <= the geometry's list capacity
    int bq;                   // queries per tile the plan was made for: LVS2_BQ (256 x 256 geometry) or LVS3_BQ
    int ntiles, tiles_per_slab, nslab, nqt;
    int debug_hot;            // -DLVS_TUNING builds only (env LVS_DEBUG_HOT), timing ablations - results are wrong
                              // unless 0: 2 skip the top-k slow path, 3 scan hits but skip insertions, 4 no wait for
                              // the staging loads.  The shipped kernel does not read this field.
    const uint32_t* pred;     // nullable: the launch is a no-op unless *pred != 0 (device-side predicate)
    int gq;                   // query tiles per XCD group (1,2,4,8,16,32); slabs per group = 32 / gq
    int lead_slabs;           // slabs walked first in 32-wide groups (see item_of_block); 0 or 1
    int no_share;             // 1: slabs do not exchange thresholds - every slab's list is its own exact top-k
    // LVS_MODE_TOPK, banded lists (kc > 0, kc < k; needs qn): a row is admitted only while its score is >= max(last slot,
    // kc-th slot - (bscale * |q| + bslack)); slots beyond the band stay empty (lvs_flat_search_keys_hi_banded)
    int kc;
    float bscale, bslack;
    // LVS_MODE_COLLECT: keys >= thr_key[q] go to bucket[q][*] (unordered, at most bucket_capacity are kept; bucket_count
    // keeps counting so that the caller sees an overflow)
    const u64* thr_key;       // [nq]
    uint32_t* bucket_count;   // [nq] zero-initialised
    u64* bucket;              // [nq][bucket_capacity]
    int bucket_capacity;
    unsigned long long* dbg;  // tuning aid (build with -DLVS_COUNT_EVENTS, run with LVS_COUNT=1): [0] block visits, [1] insertions, [2] wave-tiles, [3..5] cycles in filter / visit loop / insertions
};

hipError_t lvs_tile_launch(int mode, const LvsTileArgs& a, hipStream_t stream);

// HIP events around a dominant-kernel launch while lvs_timing_enable(1) is on (lvs_capi.hip); a no-op otherwise
struct LvsKernelTimer {
    explicit LvsKernelTimer(hipStream_t st);
    ~LvsKernelTimer();
    void* impl;
};

// ---- small-batch streaming kernel (lvs_stream.hip): nq <= 256, k <= LVS_KPASS.  One or two blocks of 32 queries per
// workgroup; beyond 64 queries 2 or 4 sibling workgroups share a corpus range through their XCD's L2. ----
struct LvsStreamArgs {
    const void* xb;
    const void* xq;
    const float* bn;
    const float* qn;
    const uint32_t* row_ids;
    uint32_t* gtau;  // [nq] zero-initialised, or seeded with a valid lower bound of every query's k-th best score
    u64* out;        // [nparts][nq][k]
    float* seed_out; // non-NULL: SEED mode - [nparts][nq] best score of every (corpus range, query) instead of lists
    long long nb, ldb, ldq, id_offset;
    int nq, k, metric;
    int nj;                  // MFMAs per 32-row block = nseg * dpad / 16
    int jper;                // dpad / 16
    int nseg;
    int seg_q[3], seg_c[3];  // column offsets (halfs) of each K segment
    int seg_b[3];            // first B-fragment index of each K segment (segments sharing query columns share fragments)
    int nbfrag;              // B fragments held in LDS per query block
    int blocks_per_wg;       // 32-row blocks per corpus range (contiguous)
    int kcap;                // list slots per query in LDS (k <= kcap <= 64), from lvs_stream_plan
    int nqb;                 // 32-query blocks per workgroup (1 .. 3), from lvs_stream_plan
    int groups;              // sibling workgroups per corpus range (1 .. 4), from lvs_stream_plan
    int nparts;              // out: corpus ranges of the launch = candidate lists per query
    int debug;               // -DLVS_TUNING builds only (env LVS_STREAM_DEBUG): 1 no MFMA / B reads, 2 no block epilogue
};

// ---- lvs_rq.hip: 97 .. 256 queries with the queries resident in registers ----
struct LvsRqArgs {
    const void* xb;
    const void* xq;
    const float* bn;
    const float* qn;
    const uint32_t* row_ids;
    uint32_t* gtau;   // [nq] zero-initialised, or seeded with a valid lower bound of every query's k-th best score
    u64* out;         // [nparts][nq][k]
    float* seed_out;  // non-NULL: SEED mode - [nparts][nq] best score of every (corpus range, query) instead of lists
    long long nb, ldb, ldq, id_offset;
    int nq, k, metric;
    int blocks_per_wg;  // 32-row blocks per corpus range (set by lvs_rq_launch)
    int nparts;         // out: corpus ranges of the launch
    int groups;         // out: query groups of LVS_RQ_GROUPQ (sibling workgroups per corpus range)
    int debug;          // -DLVS_TUNING builds only (env LVS_RQ_DEBUG), timing ablations with WRONG results: bit 0 no staging loads in
                        // the loop, bit 1 no block epilogue, bit 2 no MFMAs, bit 3 no fragment reads, bit 4 no unit barrier
    int drain_every;    // lvs_rj_kernel: every wave empties its candidate buffer every that many blocks (a power of two)
    // lvs_rj_kernel in RANGE mode (threshold join, lvs_range_join): every (query, row) with score > threshold (strict, as
    // sem_dedup.py:46) is appended to the pair list; q_row0 >= 0: self-join, pairs with row id > query row only
    long long* pair_q;
    long long* pair_j;
    float* pair_s;
    unsigned long long* pair_count;
    long long pair_capacity, q_row0, q_base;  // q_base: added to the query numbers written to pair_q (the launch's slice of the call)
    float threshold, out_scale;
};
// launch geometry (lvs_grouped_geometry), lvs_rq_fits / lvs_rj_fits and the blockIdx -> (range, group) deal: lvs_plan.h
hipError_t lvs_rq_launch(LvsRqArgs& a, int dpad, hipStream_t stream);
// ---- lvs_rj.hip: the same launches with ONE wave per SIMD and 64 queries per wave (B fragments in named accumulation registers)
hipError_t lvs_rj_launch(LvsRqArgs& a, int dpad, hipStream_t stream);  // whole 32-row blocks only: the caller adds the tail
hipError_t lvs_rj_range_launch(LvsRqArgs& a, int dpad, hipStream_t stream);  // the same geometry, RANGE epilogue (inner product)

// ---- lvs_ivf.hip: the list scan of an IVF-Flat search.  A work item is one inverted list and a tile of up to 32 of the
// (query, probe rank) pairs that probe it; the list's rows are gathered by number from the flat image. ----
#define LVS_IVF_WAVES 4
// what every scan over gathered rows reads (lvs_ivf_gather.h): the image, the lists, a chunk's queries and its work items
struct LvsIvfGatherArgs {
    const void* xb;              // the flat packed image [nb][ldb]
    const float* bn;             // [nb] |row|^2 (L2 only)
    const uint32_t* rows;        // [n] row numbers, list after list
    const int64_t* offsets;      // [nlist + 1]
    const void* xq;              // queries of this chunk [nq][ldq]
    const float* qn;             // [nq] |q|^2 (L2 only)
    const uint32_t* pairs;       // [nq * nprobe] pair numbers q * nprobe + p, bucketed by list
    const uint32_t* pair_offs;   // [nlist + 1] first pair of every list
    const uint32_t* tile_offs;   // [nlist + 1] first work item of every list (lvs_ivf_tiles_launch)
    const uint32_t* item_list;   // [work items] list of every work item
    const uint32_t* sel;         // [ceil(nb / 32)] row selector, bit r & 31 of word r >> 5 = row r takes part; NULL: every row
    long long ldb, ldq;
    int nlist, nprobe, metric;
    int jper, nseg, nbfrag;
    int seg_c[3], seg_b[3];
};
struct LvsIvfArgs {
    LvsIvfGatherArgs g;
    u64* out;                    // [nprobe][nq][k]
    int nq, k, kcap;
};
hipError_t lvs_ivf_tiles_launch(const uint32_t* pair_offs, int nlist, uint32_t* tile_offs, uint32_t* item_list,
                                hipStream_t stream);
hipError_t lvs_ivf_scan_launch(const LvsIvfArgs& a, int64_t max_items, hipStream_t stream);
hipError_t lvs_ivf_probe_ids_launch(const u64* keys, int64_t n, int32_t* out, hipStream_t stream);
hipError_t lvs_ivf_offsets_launch(const uint32_t* offs, int nlist, int64_t* out, hipStream_t stream);

// ---- lvs_ivf_range.hip: the threshold search over the lists (lvs_ivf_range_search).  The same work items and block scores;
// every (query, row) of a probed list with score > threshold goes to one pair list behind one counter. ----
struct LvsIvfRangeArgs {
    LvsIvfGatherArgs g;
    const uint32_t* q_rows;      // nullable [nq]: the row each query of this chunk IS - that row is never paired with it
    long long* out_q;            // [capacity] query number in the CALL (q_base + the chunk's)
    long long* out_j;            // [capacity] row number
    float* out_s;                // [capacity] score * out_scale
    unsigned long long* out_count;  // hits of the whole call, counted past the capacity too
    long long capacity, q_base;
    float threshold, out_scale;  // a hit: score > threshold in the kernel's (scaled) fp32 domain
};
hipError_t lvs_ivf_range_launch(const LvsIvfRangeArgs& a, int64_t max_items, hipStream_t stream);

// ---- lvs_ivf_sq8.hip: the 8-bit residual codec of IVF-SQ8 and its list scan.  A work item is one list and up to 16 of the
// (query, probe rank) pairs that probe it (half of a work item of lvs_ivf_tiles_launch); the codes are in list order. ----
#define LVS_SQ8_WAVES 4
struct LvsIvfSq8Args {
    const uint8_t* codes;        // [n][ldc] codes in list order (position p of `rows`)
    const float* rnorm;          // [n] |rhat|^2 per position (L2 only)
    const float* vmin;           // [d]
    const float* vdiff;          // [d]
    const float* cent;           // [nlist][d] fp32 centroids (the stored scale)
    const uint32_t* rows;        // [n] row numbers, list after list
    const int64_t* offsets;      // [nlist + 1]
    const void* xq;              // packed queries of this chunk [nq][ldq]
    const uint32_t* pairs;       // [nq * nprobe] pair numbers q * nprobe + p, bucketed by list
    const uint32_t* pair_offs;   // [nlist + 1]
    const uint32_t* tile_offs;   // [nlist + 1] first 32-pair work item of every list (lvs_ivf_tiles_launch)
    const uint32_t* item_list;   // [work items]
    u64* out;                    // [nprobe][nq][k]
    long long ldq;
    int nq, nlist, nprobe, k, metric, d, ldc, qsplit, qdpad, kcap;
    const uint32_t* sel;         // [ceil(nb / 32)] row selector over ROW numbers (not positions); NULL: every row
};
hipError_t lvs_ivf_sq8_encode_launch(const void* xb, int64_t ldb, int split, int xdpad, int64_t n, int d,
                                     const int64_t* offsets, int nlist, const uint32_t* rows, const float* cent,
                                     const float* vmin, const float* vdiff, uint8_t* codes, float* rnorm, hipStream_t stream);
// launches 2 x max_items blocks (max_items: lvs_ivf_max_items of the 32-pair work items)
hipError_t lvs_ivf_sq8_scan_launch(const LvsIvfSq8Args& a, int64_t max_items, hipStream_t stream);

// ---- lvs_ivf_pq.hip: the product-quantizer codec of IVF-PQ (8-bit codes) and its query-major list scan.  A workgroup is one
// query and a range of up to LVS_PQ_MAXRANGE of its probes; the codes are in list order. ----
#define LVS_PQ_WAVES 8
struct LvsIvfPqArgs {
    const uint8_t* codes;        // [n][ldc] codes in list order (position p of `rows`)
    const float* beta;           // [n] |rhat|^2 + 2 <c_l, rhat> per position (L2 only)
    const float* cent;           // [nlist][d] fp32 centroids (the stored scale)
    const uint32_t* rows;        // [n] row numbers, list after list
    const int64_t* offsets;      // [nlist + 1]
    const void* xq;              // packed queries of this chunk [nq][ldq]
    const float* lut;            // [nq][M][LVS_PQ_KSUB] lookup tables of this chunk
    const u64* coarse;           // [nq][nprobe] coarse keys (lvs_flat_search_keys over the centroids)
    u64* out;                    // [nranges][nq][k]
    long long ldq;
    int nq, nlist, nprobe, prange, k, metric, d, M, ldc, qsplit, qdpad, kcap;
    const uint32_t* sel;         // [ceil(nb / 32)] row selector over ROW numbers (not positions); NULL: every row
};
hipError_t lvs_ivf_pq_encode_launch(const void* xb, int64_t ldb, int split, int xdpad, int64_t n, int d, int M, int ksub,
                                    const int64_t* offsets, int nlist, const uint32_t* rows, const float* cent,
                                    const float* codebooks, uint8_t* codes, float* beta, hipStream_t stream);
hipError_t lvs_ivf_pq_lut_launch(const void* xq, int64_t ldq, int split, int qdpad, int64_t nq, int d, int M, int ksub,
                                 const float* codebooks, float* lut, hipStream_t stream);
// launches ceil(nprobe / prange) x nq workgroups
hipError_t lvs_ivf_pq_scan_launch(const LvsIvfPqArgs& a, hipStream_t stream);

// ---- lvs_refine.hip: exact re-ranking of up to 64 candidate rows per query (the second stage of "...,Refine(Flat)").  One
// wave per query; the rows are gathered by number from the flat image, whole rows into registers. ----
#define LVS_REFINE_WAVES 4   // queries (waves) per workgroup
#define LVS_REFINE_MAXKC 64  // candidate slots per query: one per lane
struct LvsRefineArgs {
    const void* xb;              // the flat packed image [nb][ldb]
    const float* bn;             // [nb] |row|^2 (L2 only)
    const void* xq;              // packed queries [nq][ldq]
    const float* qn;             // [nq] |q|^2 (L2 only)
    const u64* cand;             // [nq][kc] candidate keys: only the row number is read; key 0 or row >= nb: empty slot
    u64* out;                    // [nq][k]
    long long nb, nq, ldb, ldq;
    int dpad, kc, k, metric, qsplit, bsplit;
};
hipError_t lvs_refine_launch(const LvsRefineArgs& a, hipStream_t stream);

hipError_t lvs_stream_launch(LvsStreamArgs& a, hipStream_t stream);
