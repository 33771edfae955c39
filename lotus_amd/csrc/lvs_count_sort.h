// What the stable counting sorts share: the segmented radix sort of score rows (lvs_sort.hip) and the bucket sort of rows by
// an id (lvs_count_sort.hip), which serves the k-means sums, the IVF lists and the inversion of an IVF search's probes.
// Both count per (bin, chunk) in LDS, scan the counters exclusively and scatter in element order inside a chunk.
#pragma once
#include "lvs_common.h"
#include "lvs_ivf_plan.h"  // the sizes: lvs_scan_scratch_bytes, bucket_plan, lvs_bucket_workspace_bytes

// ---- exclusive scan of uint32 counters (lvs_count_sort.hip) -------------------------------------------------------
// v[0 .. total) -> its exclusive prefix sums, three launches on `stream`: per-segment scan + segment totals, scan of the totals
// (one workgroup), add.  seg: scratch of lvs_scan_scratch_bytes(total) bytes.  With `offsets`, the add also writes
// offsets[b] = v[b * nchunks] for b = 0 .. nbuckets: the start of every bucket of a (bin-major, chunk-minor) counter array.
void lvs_scan_excl_launch(uint32_t* v, long long total, uint32_t* seg, hipStream_t stream, uint32_t* offsets = nullptr,
                          int nchunks = 1, int nbuckets = 0);

// ---- bucket sort (lvs_count_sort.hip) ----------------------------------------------------------------------------
// Positions 0 .. n-1 grouped by the id in their result key (keys[i], less id_offset) or by assign[i] (exactly one of the two
// non-NULL), ascending inside a bucket; ids outside [0, k) are left out.  *rows_out [n] and *offs_out [k + 1] point into
// the workspace (lvs_bucket_workspace_bytes(n, k) bytes).
int32_t lvs_bucket_positions(const uint64_t* keys, const int64_t* assign, int64_t n, int32_t k, int64_t id_offset, void* ws,
                             int64_t ws_bytes, hipStream_t stream, const uint32_t** rows_out, const uint32_t** offs_out);
