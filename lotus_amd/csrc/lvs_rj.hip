// Join-scale batches (from a few hundred queries up: lotus/sem_ops/sem_sim_join.py:132-134 -> faiss_vs.py:67) with the queries
// resident in registers and ONE wave per SIMD - lvs_rq_kernel's successor for the calls it serves in groups of 256 queries (r6).
//
// lvs_rq_kernel keeps 32 queries per wave (192 registers of B fragments at d = 768, two waves per SIMD): every A fragment read
// from LDS feeds ONE MFMA.  Here a wave owns the whole register file of its SIMD - 256 VGPRs + 256 accumulation registers - and
// keeps 64 queries: 96 B fragments = 384 registers, of which 60 live in NAMED accumulation registers a[0:239] (hipcc's own
// allocation keeps MFMA operands in VGPRs and copies such fragments back four v_accvgpr_read per MFMA), the ring of four A
// fragments in a[240:255] (ds_read_b128 writes AGPRs, the MFMA reads both operands there), 36 B fragments and the two
// accumulators in VGPRs.  An A fragment now feeds TWO MFMAs: 0.5 LDS fragment reads per MFMA against 0.75 in the list kernel
// and 1.0 in lvs_rq_kernel, and - as there - no query traffic at all after the prologue and the corpus staged once per 256
// queries (half the list kernel's L2 -> LDS bytes per flop).  Measured on one box (tools/rj_ablate.py, 4 096 queries x 1 M x
// 768): fragment reads + MFMAs alone run at 1.53 PFLOP/s (the MFMA-only ceiling on random operands is 1.6-1.68,
// tools/probe_mfma_chain.hip); what separates the kernel from that is everything a single wave cannot hide behind a partner.
// So, unlike lvs_rq_kernel:
//   * the fragment pipeline runs ACROSS the unit barriers (a barrier certifies the unit after the one about to be computed);
//   * a block's first MFMAs take the constant 0 as C (no accumulator clears);
//   * the staging cursor lives in scalar registers and is advanced without a branch or a vector instruction: it leads the unit
//     being computed by RING - 1 units, so which k-half it is on is known when the code is generated, and "stop at the range's
//     end" is a compare + select of the byte step (see `issue_piece`); the kernel only sees WHOLE 32-row blocks - no clamping
//     arithmetic per load; the caller searches the corpus' last nb % 32 rows with lvs_rq_kernel (same arithmetic);
//   * candidates are not inserted where they are found: a lane whose score reaches its query's threshold APPENDS the key to a
//     per-wave buffer in LDS (one ballot + one write), and the buffer is drained - sorted insertions, thresholds, publication -
//     once it holds enough of them.  A wave-wide slow path per candidate (~1 500 cycles with nobody to hide it) becomes ~100
//     cycles per candidate; the thresholds lag by at most a buffer's worth, which only admits a few more candidates.
// Same operand roles, same MFMA, same k-slice order into one accumulator (the first with C = 0) as every other kernel of the
// library: keys bit-identical to the list kernel's.  Exactness of the deferred insertion: a score is dropped only when it is
// below a threshold that is the k-th best key's score of a list holding real rows of the searched set (own list or another
// workgroup's through gtau) - never above the final k-th best - and everything appended is inserted before the lists are written.
//
// The seam between two 32-row blocks, and who waits for what.  The fragment reads, the MFMAs and the staging loads are asm: the
// compiler's waitcnt pass neither counts them nor reads the s_waitcnt strings that do - inside the unit loop that is the design
// (lgkmcnt(AD - 1): three reads stay in flight, also across a block's end).  The visit and the drains are plain C++: THEIR LDS
// reads and writes are counted by the compiler, and their temporaries share registers with acc[].  Closed with a wait in an asm
// string, such a path left the pass believing that LDS results were still pending into those registers at the loop's back edge,
// and it put a full `s_waitcnt lgkmcnt(0)` in front of every block's first MFMA - behind the fragment read just issued, on every
// block, visit or not.  So every path that issues compiler-visible LDS operations (the end of `drain`, hence the overflow drain
// in `append` and the final drain; the visit in the epilogue) ends in rj_wait_lds(), the builtin the pass understands, and the
// prologue's vmcnt(0) is repeated as a builtin for the compiler's own loads of bv[] (without it the RANGE instantiations counted
// them down INSIDE the loop: vmcnt(35) ... vmcnt(0) per block, emptying the staging queue).  On the path without a candidate
// the block loop now holds no compiler-inserted wait at all (inner product; squared L2 keeps the two that its own reads of
// the rows' |y|^2 need).  The filter is ONE compare-and-branch round trip for both query blocks; which block holds the candidate
// is decided behind it.  Issuing the next unit's barrier and first read AHEAD of the filter was measured and lost 0.2 %.
#include "lvs_common.h"
#include "lvs_kstep.h"
#include "lvs_tile.h"

namespace {

using lvs_kstep::glds16;
using lvs_kstep::static_for;

#define RJ_C10(p) "a" #p "0", "a" #p "1", "a" #p "2", "a" #p "3", "a" #p "4", "a" #p "5", "a" #p "6", "a" #p "7", "a" #p "8", "a" #p "9"
#define RJ_CLOBBER_AGPRS                                                                                                          \
    "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", RJ_C10(1), RJ_C10(2), RJ_C10(3), RJ_C10(4), RJ_C10(5), RJ_C10(6), \
        RJ_C10(7), RJ_C10(8), RJ_C10(9), RJ_C10(10), RJ_C10(11), RJ_C10(12), RJ_C10(13), RJ_C10(14), RJ_C10(15), RJ_C10(16),       \
        RJ_C10(17), RJ_C10(18), RJ_C10(19), RJ_C10(20), RJ_C10(21), RJ_C10(22), RJ_C10(23), RJ_C10(24), "a250", "a251", "a252",    \
        "a253", "a254", "a255"
constexpr int RJ_A0 = 240;  // first register of the A-fragment ring (four fragments)
constexpr int RJ_AD = 4;
constexpr int RJ_CAP = 128;        // candidate buffer entries per wave
constexpr int RJ_DRAIN_EVERY = 16;  // every wave drains every that many blocks (LvsRqArgs::drain_every)

template <int I>
__device__ inline void rj_load_b(const void* p) {  // 16 bytes per lane -> a[4 I : 4 I + 3]
    asm volatile("global_load_dwordx4 a[%1:%2], %0, off" ::"v"(p), "n"(4 * I), "n"(4 * I + 3) : "memory", RJ_CLOBBER_AGPRS);
}
template <int R, int OFFSET>
__device__ inline void rj_read_a(unsigned addr) {  // A fragment -> ring register R
    static_assert(OFFSET >= 0 && OFFSET < 65536, "ds_read offset field is 16 bits");
    asm volatile("ds_read_b128 a[%1:%2], %0 offset:%3" ::"v"(addr), "n"(RJ_A0 + 4 * R), "n"(RJ_A0 + 4 * R + 3), "n"(OFFSET)
                 : "memory", RJ_CLOBBER_AGPRS);
}
// acc (+)= A(ring R) x B.  ZERO: the block's first k-slice - C is the constant 0
template <int R, int I, bool ZERO>
__device__ inline void rj_mfma_aa(f32x16& acc) {  // B = fragment I in accumulation registers
    if constexpr (ZERO)
        asm volatile("v_mfma_f32_32x32x16_f16 %0, a[%1:%2], a[%3:%4], 0"
                     : "=v"(acc)
                     : "n"(RJ_A0 + 4 * R), "n"(RJ_A0 + 4 * R + 3), "n"(4 * I), "n"(4 * I + 3)
                     : RJ_CLOBBER_AGPRS);
    else
        asm volatile("v_mfma_f32_32x32x16_f16 %0, a[%1:%2], a[%3:%4], %0"
                     : "+v"(acc)
                     : "n"(RJ_A0 + 4 * R), "n"(RJ_A0 + 4 * R + 3), "n"(4 * I), "n"(4 * I + 3)
                     : RJ_CLOBBER_AGPRS);
}
template <int R, bool ZERO>
__device__ inline void rj_mfma_av(f32x16& acc, const half8& b) {  // B in VGPRs
    if constexpr (ZERO)
        asm volatile("v_mfma_f32_32x32x16_f16 %0, a[%1:%2], %3, 0" : "=v"(acc) : "n"(RJ_A0 + 4 * R), "n"(RJ_A0 + 4 * R + 3), "v"(b) : RJ_CLOBBER_AGPRS);
    else
        asm volatile("v_mfma_f32_32x32x16_f16 %0, a[%1:%2], %3, %0" : "+v"(acc) : "n"(RJ_A0 + 4 * R), "n"(RJ_A0 + 4 * R + 3), "v"(b) : RJ_CLOBBER_AGPRS);
}
// one 1 KiB staging load: 16 bytes per lane from base (wave-uniform) + off (per lane) to LDS bytes [lds, lds + 1024) - the
// scalar-base form, spelled out (hipcc adds the base to a 64-bit copy of every lane offset instead: two registers per offset)
__device__ inline void rj_glds16(const char* base, unsigned off, unsigned lds) {
    // (readfirstlane: a wave-uniform value hipcc happens to keep in a VECTOR register is handed to an "s" operand as it is)
    const unsigned long long b = (unsigned long long)base;
    const unsigned long long bs = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned ls = (unsigned)__builtin_amdgcn_readfirstlane((int)lds);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(bs), "s"(ls) : "memory", "m0");
}
__device__ inline void rj_glds4(const void* gsrc, void* ldst) {
    __builtin_amdgcn_global_load_lds((lvs_kstep::gbl_void_t*)gsrc, (lvs_kstep::lds_void_t*)ldst, 4, 0, 0);
}
// lgkmcnt(0) as an instruction the compiler's waitcnt pass sees (gfx9 encoding: vmcnt 63, expcnt 7 = not waited for; lgkmcnt =
// bits 11:8 = 0).  It closes every path that issued compiler-visible LDS operations: a wait inside an asm string is opaque to
// that pass, which then believes results may still be pending into registers the next block overwrites (see the header).
__device__ inline void rj_wait_lds() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);
    asm volatile("" ::: "memory");
}
constexpr int rj_piece_at(int jj, int uk, int lpw) {  // staging piece p (0 .. lpw) goes out at MFMA step p * uk / (lpw + 1) + 1
    for (int p = 0; p <= lpw; ++p)
        if (jj == p * uk / (lpw + 1) + 1) return p;
    return -1;
}

#ifdef LVS_TUNING
// tuning builds: cycle / event counters of the DBG = 32 instantiation (tools/rj_ablate.py), summed over all waves
__device__ unsigned long long rj_dbg[16];
#endif

template <int NJ>
struct RjGeom {
    static constexpr int UK = NJ % 24 == 0 ? 24 : 16;  // k-slices per staged unit
    static_assert(NJ % UK == 0 && UK % RJ_AD == 0 && UK % 4 == 0, "units tile a row; the A ring closes over a unit");
    static constexpr int U = NJ / UK;
    static constexpr int ROWB = UK * 32 + 16;   // padded row of a unit (odd multiple of 16 B: conflict-free linear fragment reads)
    static constexpr int NLOAD = UK + 1;        // 1 KiB staging loads per unit (the last one half used)
    static constexpr int UB = NLOAD * 1024;     // ring slot stride
    static constexpr int LPW = UK / 4;          // full loads per wave and unit (+ the half-used one, taken in turns)
    static constexpr int NB_AGPR = 2 * NJ < 60 ? 2 * NJ : 60;  // B fragments in accumulation registers
    static constexpr int NB_VGPR = 2 * NJ - NB_AGPR;
    static constexpr int nb_ring(int ring) { return (ring - 1 + U - 1) / U + 2; }  // blocks whose side words are in flight or in use
    static constexpr int lds_bytes(int ring, int kcap) {
        return ring * UB + 256 * kcap * 8 + 8 * nb_ring(ring) * 256 + 4 * RJ_CAP * 12;
    }
    static constexpr int ring(int kcap) {
        for (int r = 7; r >= 4; --r)
            if (lds_bytes(r, kcap) <= 160 * 1024) return r;
        return 0;
    }
};

// NJ = K / 16; KCAP = list slots per query (k <= KCAP); L2: squared-L2 scores (the rows' |y|^2 ride in with the block)
// RANGE: the threshold join of sem_dedup (lvs_range_join) on the same frame - no lists, no thresholds to exchange: a score above
// the (one, constant) threshold goes straight to the global pair list
// SOLO: a top-k launch with ONE corpus range (a.nparts == 1: every workgroup owns its 256 queries over the whole shard, nobody else
// holds a list for them) - nothing to take in and nobody to publish to: no threshold side words (squared L2 keeps the rows'
// |y|^2), no side-word read or widened waits in a block's last unit, no atomicMax.  The thresholds start from the seeds in
// a.gtau and tighten from the wave's own lists in `drain`, as in the shared form - which stays correct at one range.
template <int NJ, int KCAP, bool L2, int DBG = 0, bool RANGE = false, bool SOLO = false>
__global__ __launch_bounds__(256, 1) void lvs_rj_kernel(const LvsRqArgs a) {
    static_assert(!RANGE || !L2, "the RANGE epilogue is built for inner-product scores");
    static_assert(!SOLO || (!RANGE && DBG == 0), "SOLO is a form of the shipped top-k kernel");
    using G = RjGeom<NJ>;
    constexpr int UK = G::UK, U = G::U, LPW = G::LPW, AD = RJ_AD, RING = G::ring(KCAP), NB_RING = G::nb_ring(RING);
    static_assert(RING >= 4, "LDS budget: the ring must hold the unit being read, the certified one and two in flight");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;
    u64* lists = (u64*)(smem + RING * G::UB);                         // [256][KCAP]
    float* side_all = (float*)(lists + 256 * KCAP);                   // [4 waves][NB_RING][2][64]
    u64* ckey_all = (u64*)(side_all + 8 * NB_RING * 64);              // [4][RJ_CAP] candidate keys
    uint32_t* cql_all = (uint32_t*)(ckey_all + 4 * RJ_CAP);           // [4][RJ_CAP] ... and the wave-local query (0 .. 63) of each
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* side = side_all + wave * (NB_RING * 2 * 64);
    u64* ckey = ckey_all + wave * RJ_CAP;
    uint32_t* cql = cql_all + wave * RJ_CAP;
    u64* mylists = lists + (long long)(wave * 64) * KCAP;
    const int k = a.k;
    // groups of 256 queries; the siblings of a corpus range take consecutive slots of ONE XCD (lvs_rq_kernel's deal)
    int range, group;
    if (!lvs_rq_item(blockIdx.x, a.groups, a.nparts, range, group)) return;
    const int qbase = group * 256;
    const _Float16* xq = (const _Float16*)a.xq;
    const char* xb = (const char*)a.xb;
    const long long ldb2 = a.ldb * 2;

    // ---- this wave's 64 queries -> registers: query block qb * 4 + wave of the group, fragment j; lane l = query l & 31, halfs (l >> 5) * 8
    half8 bv[G::NB_VGPR > 0 ? G::NB_VGPR : 1];
    auto qidx_of = [&](int qb) { return qbase + (qb * 4 + wave) * 32 + (lane & 31); };  // (recomputed where needed: registers)
    float tauf[2], qnv[2];
    [[maybe_unused]] uint32_t pub[2];  // the k-th key's score (ordered) this lane last saw published for its query (SOLO: the seed only)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int qi = qidx_of(qb);
        const bool valid = qi < a.nq;
        const int qrow = valid ? qi : a.nq - 1;
        const _Float16* qp = xq + (long long)qrow * a.ldq + (lane >> 5) * 8;
        static_for<NJ>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (qb == 0) {
                if constexpr (j < G::NB_AGPR) rj_load_b<(j < G::NB_AGPR ? j : 0)>(qp + j * 16);
                else bv[j - G::NB_AGPR < 0 ? 0 : j - G::NB_AGPR] = *(const half8*)(qp + j * 16);
            } else {
                if constexpr (NJ + j < G::NB_AGPR) rj_load_b<(NJ + j < G::NB_AGPR ? NJ + j : 0)>(qp + j * 16);
                else bv[NJ + j - G::NB_AGPR < 0 ? 0 : NJ + j - G::NB_AGPR] = *(const half8*)(qp + j * 16);
            }
        });
        pub[qb] = (valid && !RANGE) ? a.gtau[qi] : 0u;
        tauf[qb] = valid ? (RANGE ? a.threshold : lvs_tau(pub[qb])) : INFINITY;  // lanes without a query never hold a candidate
        qnv[qb] = L2 ? a.qn[qrow] : 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory", RJ_CLOBBER_AGPRS);  // (the loads into named registers are asm: nobody else waits for them)
    // ... and once more as an instruction the waitcnt pass sees (vmcnt 0; expcnt 7, lgkmcnt 15 = not waited for): the fragments in
    // bv[] are the compiler's own loads, and without it it counts them down in front of their first uses INSIDE the block loop -
    // vmcnt(35) ... vmcnt(0) per block in the RANGE instantiations, the last of which empties the staging queue
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if constexpr (!RANGE)
        for (int i = lane; i < 64 * KCAP; i += 64) mylists[i] = 0;

    // ---- corpus range of this workgroup, in WHOLE 32-row blocks (the caller searches the last nb % 32 rows elsewhere)
    const long long nblocks = a.nb / 32;
    const long long b0 = (long long)range * a.blocks_per_wg;
    const long long b1 = b0 + a.blocks_per_wg < nblocks ? b0 + a.blocks_per_wg : nblocks;
    if (b0 >= b1) {  // an empty range still owns its slice of the output
        const int q1 = a.nq < qbase + 256 ? a.nq : qbase + 256;
        if constexpr (!RANGE)
            for (int i = qbase * k + tid; i < q1 * k; i += 256) a.out[(long long)range * a.nq * k + i] = 0;
        return;
    }
    const int nblk = (int)(b1 - b0);
    const int total_units = nblk * U;

    // ---- staging: load m of a unit fills LDS bytes [m * 1024, + 1024) of the unit's slot, lane l the 16-byte granule
    // g = m * 64 + l = (row, piece) with 2 UK + 1 granules per padded row (the last one is the pad: it re-reads the row's last piece)
    auto src_off = [&](int m, int ln) {
        const int g = m * 64 + ln;
        int row = g / (2 * UK + 1);
        int pc = g - row * (2 * UK + 1);
        pc = pc < 2 * UK ? pc : 2 * UK - 1;
        row = row < 31 ? row : 31;  // (granules past the unit's end: lanes 32 .. 63 of the last load)
        return (unsigned)(row * (int)ldb2 + pc * 16);
    };
    unsigned soff[LPW + 1];
#pragma unroll
    for (int i = 0; i < LPW; ++i) soff[i] = src_off(wave * LPW + i, lane);
    soff[LPW] = src_off(UK, lane);
    // the staging cursor (wave-uniform, scalar registers only): the unit issued next.  It leads the unit being computed by
    // exactly RING - 1 units, so its k-half `ikh` is a compile-time constant at every call site ((kh + RING - 1) % U in `unit`,
    // n % U in the prologue): which of the two byte steps the source takes - UK * 32 to the same rows' next k-half, is_step_blk to
    // the next block's first - is decided when the code is generated, and whether it is taken at all (not past the range's end) is
    // one scalar compare + select.  No branch, no vector instruction; the LDS side keeps a byte address that wraps by compare +
    // select.  What stays a branch: the quarter-used last piece (one wave in turn) and the once-per-block side-word DMA.
    const char* is_src = xb + b0 * 32 * ldb2;
    const long long is_step_blk = 32 * ldb2 - (long long)(U - 1) * UK * 32;
    const unsigned is_dst0 = (unsigned)(unsigned long long)ring + (unsigned)(wave * (LPW * 1024));  // this wave's share of slot 0
    const unsigned is_dst_end = is_dst0 + (unsigned)(RING * G::UB);
    const unsigned is_dst_last = (unsigned)((UK - wave * LPW) * 1024);  // from this wave's share to the slot's last (quarter-used) KiB
    unsigned is_dst = is_dst0;
    int is_n = 0;
    [[maybe_unused]] const float* is_bn = L2 ? a.bn + b0 * 32 : nullptr;  // |y|^2 of the issued unit's block (squared L2)
    [[maybe_unused]] unsigned is_side = 0;  // float offset of that block's side words: (block % NB_RING) * 128
    auto issue_piece = [&](auto pc, auto ikhc) {
        constexpr int i = decltype(pc)::value;
        constexpr int ikh = decltype(ikhc)::value;  // the k-half of unit is_n (is_n % U)
        if constexpr (i < LPW) {
            rj_glds16(is_src, soff[i], is_dst + (unsigned)(i * 1024));
        } else {
            if ((is_n & 3) == wave) rj_glds16(is_src, soff[LPW], is_dst + is_dst_last);
            constexpr bool side_unit = !RANGE && (!SOLO || L2) && ikh == 0;  // a block's first unit, in a form that has side words
            if (side_unit && is_n < total_units) {
                // the block's side words, one 4-byte DMA per query block: lanes 0 .. 31 -> |y|^2 of its rows (any valid word under
                // inner product), lanes 32 .. 63 -> the shared thresholds of this wave's queries as the other workgroups left them
                // (inner product: ONE 4-byte DMA - words 0 .. 31 the thresholds of query block 0, words 32 .. 63 those of query
                // block 1; squared L2: two - |y|^2 | thresholds 0, then thresholds 1 in the upper half of the second)
                if constexpr (SOLO) {  // (squared L2 only: the rows' |y|^2, in both halves of the one word row the epilogue reads)
                    rj_glds4(is_bn + (lane & 31), side + is_side);
                } else if constexpr (L2) {
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb) {
                        const int q = qidx_of(qb) < a.nq ? qidx_of(qb) : 0;
                        const void* p = lane < 32 ? (const void*)(is_bn + (lane & 31)) : (const void*)(a.gtau + q);
                        rj_glds4(p, side + is_side + qb * 64);
                    }
                } else {
                    const int qi = qidx_of(lane >> 5);
                    rj_glds4(a.gtau + (qi < a.nq ? qi : 0), side + is_side);
                }
            }
            // advance the cursor; past the range's end the last unit is loaded again (into a free slot, never read): once `more`
            // is false it stays false, so the compile-time phase moves nothing from then on
            const bool more = is_n + 1 < total_units;
            if constexpr (ikh == U - 1) {
                is_src += more ? is_step_blk : 0ll;
                if constexpr (!RANGE && (!SOLO || L2)) {
                    if constexpr (L2) is_bn += more ? 32 : 0;
                    const unsigned nside = is_side + 128 == (unsigned)(NB_RING * 128) ? 0u : is_side + 128;
                    is_side = more ? nside : is_side;
                }
            } else {
                is_src += more ? (long long)(UK * 32) : 0ll;
            }
            ++is_n;
            is_dst = is_dst + (unsigned)G::UB == is_dst_end ? is_dst0 : is_dst + (unsigned)G::UB;
            // (the new cursor is due HERE, in the shadow of this step's MFMAs: left alone, the compiler sinks the advance of a
            // block's last unit behind the epilogue, where nothing hides it)
            asm volatile("" : "+s"(is_src), "+s"(is_dst), "+s"(is_n));
            if constexpr (!RANGE && (!SOLO || L2) && ikh == U - 1) asm volatile("" : "+s"(is_side));
            if constexpr (L2 && ikh == U - 1) asm volatile("" : "+s"(is_bn));
        }
    };
    // ---- fragment reads: lane (r = l & 31, h = l >> 5) reads bytes [(2 jj + h) * 16, + 16) of padded row r: lane base + jj * 32
    unsigned o_base = (unsigned)(unsigned long long)ring + (unsigned)((lane & 31) * G::ROWB + (lane >> 5) * 16);
    int slot = 0;
    f32x16 acc[2];
    const unsigned side_lds = (unsigned)(unsigned long long)side + (unsigned)((lane & 31) * 4);

    // ---- deferred insertion: candidates wait in the wave's buffer; `drain` inserts them (wave-cooperative sorted insertion: lane
    // j < k owns slot j of the query's list - no lock, the list is this wave's), tightens the lanes' thresholds and publishes
    int count = 0;  // wave-uniform
    [[maybe_unused]] unsigned long long d_visit = 0, d_drain = 0, d_bar = 0, d_nvisit = 0, d_ndrain = 0, d_ncand = 0, d_epi = 0;  // (tuning builds: DBG = 32)
    auto drain = [&]() {
        const unsigned long long t_d0 = (DBG & 32) ? __builtin_amdgcn_s_memtime() : 0;
        d_ndrain += 1;
        d_ncand += count;
        uint32_t best[2] = {0u, 0u};
        const int grp = lane >> 4, slot16 = lane & 15;
        for (int i0 = 0; i0 < count; i0 += 64) {
            // every lane fetches ONE waiting entry (a single LDS round trip for up to 64 of them); then FOUR entries per round:
            // the 16 lanes of group g own the list slots of entry i + g's query (k <= 16), so one list read + write serves four
            // insertions - unless two of the four hit the same query, which then take their turns
            const int n = count - i0 < 64 ? count - i0 : 64;
            u64 ek = 0;
            uint32_t eq = 0xFFFFFFFFu;
            if (lane < n) {
                ek = ckey[i0 + lane];
                eq = cql[i0 + lane];
            }
            if constexpr (L2) {  // (squared L2 has no registers to spare for the four-at-a-time form: one entry per round)
                for (int i = 0; i < n; ++i) {
                    const u64 ukey = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ek >> 32), i) << 32) |
                                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ek, i);
                    const int uq = __builtin_amdgcn_readlane((int)eq, i);
                    u64* UL = mylists + uq * KCAP;
                    u64 mine = 0;
                    if (lane < k) mine = UL[lane];
                    u64 prev = ((u64)(uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)(mine >> 32), 0x138, 0xf, 0xf, false) << 32) |
                               (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)mine, 0x138, 0xf, 0xf, false);
                    if (lane == 0) prev = ~0ull;
                    u64 newv = 0;
                    if (lane < k) newv = mine > ukey ? mine : (prev > ukey ? ukey : prev);
                    if (lane < k) UL[lane] = newv;
                    const uint32_t ntau = __builtin_amdgcn_readlane((uint32_t)(newv >> 32), k - 1);
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
                        if (qb * 32 + (lane & 31) == uq) best[qb] = ntau > best[qb] ? ntau : best[qb];
                }
            } else
            for (int i = 0; i < n; i += 4) {
                uint32_t sq[4];  // (scalar) the four entries' queries; 0xFFFFFFFF = no entry
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) sq[gg] = i + gg < n ? (uint32_t)__builtin_amdgcn_readlane((int)eq, (i + gg) & 63) : 0xFFFFFFFFu;
                const bool clash = (sq[0] == sq[1] && sq[1] != 0xFFFFFFFFu) || (sq[0] == sq[2] && sq[2] != 0xFFFFFFFFu) ||
                                   (sq[0] == sq[3] && sq[3] != 0xFFFFFFFFu) || (sq[1] == sq[2] && sq[2] != 0xFFFFFFFFu) ||
                                   (sq[1] == sq[3] && sq[3] != 0xFFFFFFFFu) || (sq[2] == sq[3] && sq[3] != 0xFFFFFFFFu);
                const int e = (i + grp) & 63;
                const u64 ukey = ((u64)(uint32_t)__shfl((int)(uint32_t)(ek >> 32), e, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)ek, e, 64);
                const uint32_t uq = grp == 0 ? sq[0] : (grp == 1 ? sq[1] : (grp == 2 ? sq[2] : sq[3]));
                for (int turn = 0; turn < (clash ? 4 : 1); ++turn) {
                    const bool act = uq != 0xFFFFFFFFu && slot16 < k && (!clash || grp == turn);
                    u64* UL = mylists + (act ? uq : 0u) * KCAP;
                    u64 mine = 0;
                    if (act) mine = UL[slot16];
                    // the neighbour slot through a row shift instead of a second LDS read
                    u64 prev = ((u64)(uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)(mine >> 32), 0x111, 0xf, 0xf, false) << 32) |
                               (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)mine, 0x111, 0xf, 0xf, false);
                    if (slot16 == 0) prev = ~0ull;
                    const u64 newv = mine > ukey ? mine : (prev > ukey ? ukey : prev);
                    if (act) UL[slot16] = newv;
#pragma unroll
                    for (int gg = 0; gg < 4; ++gg) {
                        if (sq[gg] == 0xFFFFFFFFu || (clash && gg != turn)) continue;  // (wave-uniform)
                        const uint32_t ntau = __builtin_amdgcn_readlane((uint32_t)(newv >> 32), gg * 16 + k - 1);
#pragma unroll
                        for (int qb = 0; qb < 2; ++qb)
                            if ((uint32_t)(qb * 32 + (lane & 31)) == sq[gg]) best[qb] = ntau > best[qb] ? ntau : best[qb];
                    }
                }
            }
        }
        count = 0;
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            if constexpr (SOLO) {  // (best = 0: no list of this lane's query filled up in this drain)
                if (best[qb]) tauf[qb] = fmaxf(tauf[qb], lvs_tau(best[qb]));
            } else if (best[qb] > pub[qb]) {  // a full list's k-th key is published to the other workgroups (fire and forget)
                tauf[qb] = fmaxf(tauf[qb], lvs_tau(best[qb]));
                pub[qb] = best[qb];
                if (lane < 32 && !(DBG & 512)) atomicMax(&a.gtau[qidx_of(qb)], best[qb]);
            }
        }
        rj_wait_lds();  // the unit loop counts its fragment reads from zero
        if (DBG & 32) d_drain += __builtin_amdgcn_s_memtime() - t_d0;
    };
    // what the other workgroups have found meanwhile (a lower bound of the k-th best over ALL rows), as it rode in with the block
    [[maybe_unused]] auto take_shared = [&](int qb, uint32_t g) {
        if (g > pub[qb]) {
            pub[qb] = g;
            tauf[qb] = fmaxf(tauf[qb], lvs_tau(g));
        }
    };
    // The lanes whose scores of query block qb reach their thresholds append them to the wave's buffer; lane holds query
    // qidx_of(qb), rows row0 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    auto append = [&](const f32x16& v, int qb, long long row0) {
        // all sixteen "which lanes hold a candidate in register r?" masks first, back to back: a compare whose result steers a
        // scalar branch costs ~45 cycles of VALU -> SALU latency, and one per register (the obvious loop) made a visit ~1 400
        // cycles on a wave that has nobody to hide behind (stamps: tools/rj_ablate.py).  ONE drain site behind the loop (a full
        // buffer: hundreds of equal scores in a block) - inlined at every register it made the visit 25 KB of code, walked once
        // per visit straight out of a cold instruction cache.
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {  // (four masks at a time, back to back: see above)
            u64 m[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = __ballot(v[g4 * 4 + e] >= tauf[qb]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = g4 * 4 + e;
                if (m[e] == 0) continue;
                if (count + __popcll(m[e]) > RJ_CAP) {  // (only with hundreds of equal scores in a block)
                    drain();
                    m[e] = __ballot(v[r] >= tauf[qb]);
                    if (m[e] == 0) continue;
                }
                const int pos = count + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m[e] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[e], 0u));
                if ((m[e] >> lane) & 1) {
                    const long long row = row0 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
                    ckey[pos] = lvs_pack_key(v[r], (uint32_t)(row + a.id_offset));
                    cql[pos] = (uint32_t)(qb * 32 + (lane & 31));
                }
                count += __popcll(m[e]);
            }
        }
    };
    // every wave drains at the SAME blocks: a drain (hundreds of cycles per candidate) holds up the other three waves at the next
    // barrier, so four drains at four different moments cost the workgroup four times what four at once do
    auto block_end = [&](int blk) {
        if constexpr (DBG & 128) {
            if ((blk & (a.drain_every - 1)) == a.drain_every - 1) count = 0;
        } else {
            if (count > 0 && (count >= RJ_CAP - 64 || (blk & (a.drain_every - 1)) == a.drain_every - 1)) drain();
        }
    };
    // ---- block epilogue: 32 rows x this wave's 64 queries.  With one wave per SIMD nothing hides it, so as much of it as
    // possible has already happened inside the block's last MFMA steps (see `unit`): the side words are in registers (gsh) and the
    // thresholds the other workgroups published are taken in.  Left for here: the wait states behind the last MFMA, the lanes'
    // maxima, "does any lane hold a candidate?" - and, rarely, the visit.
    [[maybe_unused]] unsigned gsh[2] = {0u, 0u};
    auto epilogue = [&](int blk) {
        const long long row0 = (b0 + blk) * 32;
        const unsigned long long t_e0 = (DBG & 32) ? __builtin_amdgcn_s_memtime() : 0;
        // (inline-asm MFMAs are invisible to hipcc's hazard recogniser: the wait states between the block's last MFMA and the
        // first VALU read of its result are spelled out)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]));
        if constexpr (L2) {
            const float* bnb = side + (blk % NB_RING) * 2 * 64 + 4 * (lane >> 5);  // |y|^2 of this lane's 16 rows
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const f32x4 bn4 = *(const f32x4*)(bnb + 8 * m);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb)
                        acc[qb][m * 4 + e] = -fmaxf((qnv[qb] + bn4[e]) - 2.0f * acc[qb][m * 4 + e], 0.f);
            }
        }
        if constexpr (RANGE) {
            // strict ">" as the reference compares (sem_dedup.py:46); a self-join keeps the pairs with row id > query row
            const float mx[2] = {lvs_max16(acc[0]), lvs_max16(acc[1])};
            if (__any(mx[0] > tauf[0] || mx[1] > tauf[1]))  // ONE round trip on the common path; per query block only behind it
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                if (!__any(mx[qb] > tauf[qb])) continue;
                const long long qg = qidx_of(qb);
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    u64 m[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) m[e] = __ballot(acc[qb][g4 * 4 + e] > tauf[qb]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (m[e] == 0) continue;
                        const int r = g4 * 4 + e;
                        const long long jg = row0 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2) + a.id_offset;
                        if (((m[e] >> lane) & 1) && !(a.q_row0 >= 0 && jg <= a.q_row0 + qg)) {
                            const unsigned long long pos = atomicAdd(a.pair_count, 1ull);  // (keeps counting past the capacity)
                            if ((long long)pos < a.pair_capacity) {
                                a.pair_q[pos] = qg + a.q_base;
                                a.pair_j[pos] = jg;
                                a.pair_s[pos] = acc[qb][r] * a.out_scale;
                            }
                        }
                    }
                }
            }
        } else if constexpr (!(DBG & 4)) {
            const unsigned long long t_v0 = (DBG & 32) ? __builtin_amdgcn_s_memtime() : 0;
            // ONE "does any lane of either query block hold a candidate?" round trip on the common path; which block - the
            // same compares against the same thresholds, block 1's after block 0's visit as before - only behind it
            const float mx[2] = {lvs_max16(acc[0]), lvs_max16(acc[1])};
            if (__any(mx[0] >= tauf[0] || mx[1] >= tauf[1])) {
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
                    if (__any(mx[qb] >= tauf[qb])) {
                        if constexpr (!(DBG & 64)) append(acc[qb], qb, row0);
                        else count += 1;
                    }
                // (LDS writes of its own only behind a visit: the unit loop counts its fragment reads from zero)
                if constexpr (!(DBG & 64)) rj_wait_lds();
                if (DBG & 32) {
                    d_visit += __builtin_amdgcn_s_memtime() - t_v0;
                    d_nvisit += 1;
                }
            }
        } else {
            if (__any(lvs_max16(acc[0]) >= 3.0e38f) || __any(lvs_max16(acc[1]) >= 3.0e38f)) count = 1;
        }
        if constexpr (!RANGE) block_end(blk);
        if (DBG & 32) d_epi += __builtin_amdgcn_s_memtime() - t_e0;
    };

    // One unit of block `blk`.  In the block's LAST unit the epilogue's memory part rides along: step UK - 7 reads the block's side
    // words (ONE more LDS read in flight: the counted waits of the next three steps allow for it), steps UK - 3 / UK - 2 take the
    // thresholds in.  SOLO has no such unit: every unit keeps the plain lgkmcnt(AD - 1) schedule.
    auto unit = [&](auto khc, int blk) {
        constexpr int kh = decltype(khc)::value;
        constexpr bool F = kh == U - 1 && !(DBG & 2) && !(DBG & 256) && !RANGE && !SOLO;
        constexpr int JS = UK - 7;  // the step that reads the side words
        const unsigned o_next = o_base + (slot + 1 == RING ? (unsigned)(-(RING - 1) * G::UB) : (unsigned)G::UB);
        static_for<UK>([&](auto jc) {
            constexpr int jj = decltype(jc)::value;
            constexpr int ahead = jj + AD - 1;
            if constexpr (ahead < UK) rj_read_a<ahead % AD, (ahead < UK ? ahead : 0) * 32>(o_base);
            else rj_read_a<ahead % AD, (ahead >= UK ? ahead - UK : 0) * 32>(o_next);  // the next unit's slot: certified at this unit's barrier
            if constexpr (F && jj == JS)
            {
                if constexpr (L2)
                    asm volatile("ds_read2_b32 %0, %1 offset0:32 offset1:96" : "=v"(*(unsigned long long*)gsh) : "v"(side_lds + (unsigned)((blk % NB_RING) * 512)) : "memory");
                else
                    asm volatile("ds_read2_b32 %0, %1 offset0:0 offset1:32" : "=v"(*(unsigned long long*)gsh) : "v"(side_lds + (unsigned)((blk % NB_RING) * 512)) : "memory");
            }
            constexpr int piece = rj_piece_at(jj, UK, LPW);
            if constexpr (piece >= 0 && !(DBG & 1)) issue_piece(std::integral_constant<int, piece>{}, std::integral_constant<int, (kh + RING - 1) % U>{});
            __builtin_amdgcn_sched_barrier(0);
            constexpr int extra = (F && jj >= JS && jj < JS + AD - 1) ? 1 : 0;
            if constexpr (F && jj == JS + AD - 1) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(*(unsigned long long*)gsh) : "n"(AD - 1) : "memory");
            else asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(AD - 1 + extra) : "memory");
            constexpr bool zero = kh == 0 && jj == 0;
            constexpr int f0 = kh * UK + jj, f1 = NJ + kh * UK + jj;
            if constexpr (f0 < G::NB_AGPR) rj_mfma_aa<jj % AD, (f0 < G::NB_AGPR ? f0 : 0), zero>(acc[0]);
            else rj_mfma_av<jj % AD, zero>(acc[0], bv[f0 - G::NB_AGPR < 0 ? 0 : f0 - G::NB_AGPR]);
            if constexpr (f1 < G::NB_AGPR) rj_mfma_aa<jj % AD, (f1 < G::NB_AGPR ? f1 : 0), zero>(acc[1]);
            else rj_mfma_av<jj % AD, zero>(acc[1], bv[f1 - G::NB_AGPR < 0 ? 0 : f1 - G::NB_AGPR]);
            if constexpr (F && jj == UK - 3) take_shared(0, gsh[0]);
            if constexpr (F && jj == UK - 2) take_shared(1, gsh[1]);
            __builtin_amdgcn_sched_barrier(0);
        });
        slot = slot + 1 == RING ? 0 : slot + 1;
        o_base = o_next;
    };

    // ---- prologue: RING - 1 units in flight, unit 0 certified by a barrier of its own, its first fragments read
    static_for<RING - 1>([&](auto nc) {
        static_for<LPW + 1>([&](auto pc) { issue_piece(pc, std::integral_constant<int, decltype(nc)::value % U>{}); });
    });
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RING - 2) * LPW) : "memory");
    __builtin_amdgcn_s_barrier();
    static_for<AD - 1>([&](auto jc) {
        constexpr int jj = decltype(jc)::value;
        rj_read_a<jj % AD, jj * 32>(o_base);
    });
    for (int blk = 0; blk < nblk; ++blk) {
        static_for<U>([&](auto khc) {
            // unit n + 1 has landed once this wave's loads of the RING - 3 younger units are all that is in flight (the half-used
            // load and the side words ride in the same queue: the wait is only more conservative); the barrier makes that true
            // for every wave's share and tells everybody that unit n - 1's slot is free again
            const unsigned long long t_b0 = (DBG & 32) ? __builtin_amdgcn_s_memtime() : 0;
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RING - 3) * LPW) : "memory");
            if constexpr (!(DBG & 16)) __builtin_amdgcn_s_barrier();
            if (DBG & 32) d_bar += __builtin_amdgcn_s_memtime() - t_b0;
            unit(khc, blk);
        });
        if constexpr (!(DBG & 2)) epilogue(blk);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the clamped tail loads still target the ring; the last fragment reads
    if constexpr (RANGE) return;
    drain();
#ifdef LVS_TUNING
    if ((DBG & 32) && lane == 0) {
        atomicAdd(&rj_dbg[0], d_visit);
        atomicAdd(&rj_dbg[1], d_drain);
        atomicAdd(&rj_dbg[2], d_bar);
        atomicAdd(&rj_dbg[3], d_nvisit);
        atomicAdd(&rj_dbg[4], d_ndrain);
        atomicAdd(&rj_dbg[5], d_ncand);
        atomicAdd(&rj_dbg[6], d_epi);
        atomicAdd(&rj_dbg[7], (unsigned long long)nblk);
        atomicAdd(&rj_dbg[8], 1ull);
    }
#endif
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < 64 * k; i += 64) {
        const int ql = i / k, j = i - ql * k;
        const int q = qbase + ((ql >> 5) * 4 + wave) * 32 + (ql & 31);
        if (q < a.nq) a.out[((long long)range * a.nq + q) * k + j] = mylists[ql * KCAP + j];
    }
    if (!SOLO && lane < 32) {
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const uint32_t lo = (uint32_t)(mylists[(qb * 32 + lane) * KCAP + k - 1] >> 32);
            if (lo && qidx_of(qb) < a.nq) atomicMax(&a.gtau[qidx_of(qb)], lo);
        }
    }
}

template <int NJ, int KCAP, bool L2, int DBG = 0, bool RANGE = false, bool SOLO = false>
hipError_t rj_launch_k(const LvsRqArgs& a, int grid, hipStream_t stream) {
    using G = RjGeom<NJ>;
    const size_t lds = (size_t)G::lds_bytes(G::ring(KCAP), KCAP);  // (SOLO keeps the side-word region: RING is the same without it)
    return lvs_launch_lds<lvs_rj_kernel<NJ, KCAP, L2, DBG, RANGE, SOLO>>(dim3(grid), dim3(256), lds, stream, a);
}
template <int NJ, int KCAP, bool L2>
hipError_t rj_launch_form(const LvsRqArgs& a, int grid, hipStream_t stream, bool solo) {
    return solo ? rj_launch_k<NJ, KCAP, L2, 0, false, true>(a, grid, stream) : rj_launch_k<NJ, KCAP, L2>(a, grid, stream);
}
// solo: the launch has one corpus range (the shared form is correct there too: the tuning ablations below keep it)
template <int NJ>
hipError_t rj_launch_nj(const LvsRqArgs& a, int grid, hipStream_t stream, bool solo) {
    const bool l2 = a.metric == LVS_METRIC_L2;
#ifdef LVS_TUNING
    if (NJ == 48 && !l2 && a.k <= 10) {  // timing ablations (LVS_RQ_DEBUG; WRONG results): 1 no staging loads, 2 no epilogue, 4 + filter only, 16 no barrier
        switch ((int)lvs_tune("LVS_RQ_DEBUG", 0)) {
            case 1: return rj_launch_k<NJ, 10, false, 1>(a, grid, stream);
            case 2: return rj_launch_k<NJ, 10, false, 2>(a, grid, stream);
            case 3: return rj_launch_k<NJ, 10, false, 3>(a, grid, stream);
            case 6: return rj_launch_k<NJ, 10, false, 6>(a, grid, stream);
            case 18: return rj_launch_k<NJ, 10, false, 18>(a, grid, stream);
            case 19: return rj_launch_k<NJ, 10, false, 19>(a, grid, stream);
            case 32: return rj_launch_k<NJ, 10, false, 32>(a, grid, stream);
            case 64: return rj_launch_k<NJ, 10, false, 64>(a, grid, stream);
            case 512: return rj_launch_k<NJ, 10, false, 512>(a, grid, stream);
            case 128: return rj_launch_k<NJ, 10, false, 128>(a, grid, stream);
            case 192: return rj_launch_k<NJ, 10, false, 192>(a, grid, stream);
            case 448: return rj_launch_k<NJ, 10, false, 448>(a, grid, stream);
            default: break;
        }
    }
#endif
    if (a.k <= 10) return l2 ? rj_launch_form<NJ, 10, true>(a, grid, stream, solo) : rj_launch_form<NJ, 10, false>(a, grid, stream, solo);
    return l2 ? rj_launch_form<NJ, LVS_RQ_KMAX, true>(a, grid, stream, solo) : rj_launch_form<NJ, LVS_RQ_KMAX, false>(a, grid, stream, solo);
}

}  // namespace

#ifdef LVS_TUNING
// tuning builds: read and clear the DBG = 32 counters (visit / drain / barrier cycles, visits, drains, candidates, epilogue cycles,
// blocks, waves)
extern "C" int32_t lvs_rj_debug_read(unsigned long long* out16) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(rj_dbg), sizeof(unsigned long long) * 16) != hipSuccess) return LVS_EDEVICE;
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(rj_dbg), z, sizeof(z)) != hipSuccess) return LVS_EDEVICE;
    return LVS_OK;
}
#endif

static hipError_t rj_launch_any(LvsRqArgs& a, int dpad, hipStream_t stream, bool range_mode);
// a.nb rows are searched in whole 32-row blocks: the caller runs the last a.nb % 32 rows through lvs_rq_launch (one more list per
// query).  On return a.nparts = candidate lists per query in a.out ([nparts][nq][k]).
hipError_t lvs_rj_launch(LvsRqArgs& a, int dpad, hipStream_t stream) { return rj_launch_any(a, dpad, stream, false); }
// The threshold join on the same launch geometry (whole 32-row blocks; inner product; a.pair_* / a.threshold / a.q_row0 set)
hipError_t lvs_rj_range_launch(LvsRqArgs& a, int dpad, hipStream_t stream) { return rj_launch_any(a, dpad, stream, true); }
static hipError_t rj_launch_any(LvsRqArgs& a, int dpad, hipStream_t stream, bool range_mode) {
    LvsGroupedGeom g;
    if (!lvs_grouped_geometry(a.nq, a.nb / 32, g)) return hipErrorInvalidValue;
    a.groups = g.groups;
    a.blocks_per_wg = g.blocks_per_wg;
    a.nparts = g.nparts;
    a.drain_every = (int)lvs_tune("LVS_RJ_EVERY", RJ_DRAIN_EVERY);
    if (a.drain_every < 1 || (a.drain_every & (a.drain_every - 1))) a.drain_every = RJ_DRAIN_EVERY;
    const int grid = lvs_rq_grid(a.groups, a.nparts);
    const bool solo = !range_mode && a.nparts == 1 && lvs_tune("LVS_RJ_SOLO", LVS_RJ_SOLO_DEFAULT) != 0;
    if (range_mode) {
        if (a.metric != LVS_METRIC_IP) return hipErrorInvalidValue;
        switch (dpad / 16) {
            case 48: return rj_launch_k<48, 10, false, 0, true>(a, grid, stream);
            case 32: return rj_launch_k<32, 10, false, 0, true>(a, grid, stream);
            case 24: return rj_launch_k<24, 10, false, 0, true>(a, grid, stream);
            case 16: return rj_launch_k<16, 10, false, 0, true>(a, grid, stream);
            default: return hipErrorInvalidValue;
        }
    }
    switch (dpad / 16) {
        case 48: return rj_launch_nj<48>(a, grid, stream, solo);
        case 32: return rj_launch_nj<32>(a, grid, stream, solo);
        case 24: return rj_launch_nj<24>(a, grid, stream, solo);
        case 16: return rj_launch_nj<16>(a, grid, stream, solo);
        default: return hipErrorInvalidValue;
    }
}
