// Shared device/host helpers for liblotus_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lotus_hip.h"
#include "lvs_plan.h"  // host planner: geometry constants, lvs_round_up / lvs_ceil_div, lvs_tune

typedef unsigned long long u64;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- result keys -------------------------------------------------------------------------------------------
// key = ord32(score where larger is better) << 32 | (0xFFFFFFFF - id); descending key order is
// (score best-first, id ascending) - the total order the oracle uses (oracle/flat.py pack_keys).
__host__ __device__ inline uint32_t lvs_ord32(float f) {
    f = f + 0.0f;  // fold -0.0 onto +0.0 so equal floats get equal keys
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u >> 31) ? ~u : (u ^ 0x80000000u);
}
__host__ __device__ inline float lvs_unord32(uint32_t o) {
    uint32_t u = (o >> 31) ? (o ^ 0x80000000u) : ~o;
    return __builtin_bit_cast(float, u);
}
__host__ __device__ inline u64 lvs_pack_key(float better, uint32_t id) {
    return ((u64)lvs_ord32(better) << 32) | (u64)(0xFFFFFFFFu - id);
}

// ---- wave64 helpers ----------------------------------------------------------------------------------------
__device__ inline u64 lvs_shfl_xor_u64(u64 v, int mask) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return ((u64)hi << 32) | lo;
}
__device__ inline u64 lvs_shfl_u64(u64 v, int src) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl(lo, src, 64);
    hi = __shfl(hi, src, 64);
    return ((u64)hi << 32) | lo;
}
// Bitonic sort of one u64 per lane across the 64 lanes of a wave, descending in lane order.
__device__ inline u64 lvs_wave_sort_desc(u64 v, int lane) {
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            u64 o = lvs_shfl_xor_u64(v, stride);
            bool up = (lane & size) == 0;  // size == 64: always true -> whole wave descending
            bool lower = (lane & stride) == 0;
            u64 mx = v > o ? v : o, mn = v > o ? o : v;
            v = (lower == up) ? mx : mn;
        }
    }
    return v;
}
// `v` is bitonic across the wave; finish into descending order.
__device__ inline u64 lvs_wave_bitonic_merge_desc(u64 v, int lane) {
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        u64 o = lvs_shfl_xor_u64(v, stride);
        bool lower = (lane & stride) == 0;
        u64 mx = v > o ? v : o, mn = v > o ? o : v;
        v = lower ? mx : mn;
    }
    return v;
}

// Scores are finite or -inf, never NaN, so the maxima need none of fmaxf's canonicalisation (hipcc emits one extra
// `v_max_f32 x, x` per MFMA output to quiet signalling NaNs): v_max3_f32 directly - 8 instructions for 16 values.
__device__ inline float lvs_max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ inline float lvs_max16(const f32x16& v) {
    const float a = lvs_max3(v[0], v[1], v[2]), b = lvs_max3(v[3], v[4], v[5]), c = lvs_max3(v[6], v[7], v[8]);
    const float d = lvs_max3(v[9], v[10], v[11]), e = lvs_max3(v[12], v[13], v[14]);
    return lvs_max3(lvs_max3(a, b, c), lvs_max3(d, e, v[15]), v[15]);
}
// the score a list's last slot stands for: an empty slot (ord 0) admits everything
__device__ __forceinline__ float lvs_tau(uint32_t ord) { return ord == 0 ? -INFINITY : lvs_unord32(ord); }
__device__ __forceinline__ float lvs_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float lvs_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// Wave-cooperative sorted insertion into descending lists of k keys in LDS (lists [slots][KCAP], one lock per slot: the
// waves of a workgroup share the lists).  pm is the ballot of the lanes that hold a key; every such key goes, one at a time,
// into the list of its lane's slot: the key and slot are broadcast, lane 0 takes the list's lock, lane j < k reads slots j
// and j - 1 and writes the shifted slot j, lane 0 unlocks; lanes of the same slot raise their threshold tauf to the list's
// new last slot.  lvs_stream_kernel and lvs_ivf_pq_scan_kernel carry the same text in place (the call changes their code).
__device__ __forceinline__ void lvs_list_insert(unsigned long long pm, u64 key, int slot, u64* lists, int KCAP, uint32_t* locks,
                                                int k, int lane, float& tauf) {
    while (pm) {
        const int src = __ffsll((long long)pm) - 1;
        pm &= pm - 1;
        const uint32_t klo = __builtin_amdgcn_readlane((uint32_t)key, src);
        const uint32_t khi = __builtin_amdgcn_readlane((uint32_t)(key >> 32), src);
        const u64 ukey = ((u64)khi << 32) | klo;
        const int uq = __builtin_amdgcn_readlane(slot, src);
        u64* UL = lists + uq * KCAP;
        u64 mine = 0, prev = ~0ull;
        for (;;) {
            uint32_t seen = 0;
            if (lane == 0)
                __hip_atomic_compare_exchange_strong(&locks[uq], &seen, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_WORKGROUP);
            asm volatile("" ::: "memory");
            if (lane < k) {
                mine = UL[lane];
                if (lane > 0) prev = UL[lane - 1];
            }
            if (__builtin_amdgcn_readfirstlane(seen) == 0) break;
        }
        u64 newv = 0;
        if (lane < k) newv = mine > ukey ? mine : (prev > ukey ? ukey : prev);
        __builtin_amdgcn_wave_barrier();
        if (lane < k) UL[lane] = newv;
        const uint32_t ntau = __builtin_amdgcn_readlane((uint32_t)(newv >> 32), k - 1);
        asm volatile("" ::: "memory");  // slot writes stay ahead of the unlock (LDS is in-order per wave)
        if (lane == 0) __hip_atomic_store(&locks[uq], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (slot == uq) tauf = fmaxf(tauf, lvs_tau(ntau));
    }
}

// ---- the shared head and tail of the IVF-Flat and IVF-SQ8 list scans (lvs_ivf.hip, lvs_ivf_sq8.hip) -------------------------
// A workgroup of THREADS holds a tile of TQ (query, probe rank) pairs: their lists [TQ][KCAP], locks, queries and ranks in LDS.
// (The stretch between the two - threshold refresh, best, per-row insertion - stays in each kernel: as a helper it changes
// the instructions of both, profiles/kernel_plumbing_isa_check.md.)
// tile begin: pair numbers q * nprobe + p of the tile's npair pairs (pairs[p0 ..]) -> slot_q / slot_p; lists and locks cleared
template <int TQ, int THREADS>
__device__ __forceinline__ void lvs_ivf_tile_begin(const uint32_t* pairs, uint32_t p0, int npair, int nprobe, int tid, u64* lists,
                                                   int KCAP, uint32_t* locks, int* slot_q, int* slot_p) {
    if (tid < TQ) {
        const uint32_t pr = pairs[p0 + (tid < npair ? tid : 0)];  // empty slots repeat the first pair (never written)
        slot_q[tid] = (int)(pr / (uint32_t)nprobe);
        slot_p[tid] = (int)(pr % (uint32_t)nprobe);
    }
    for (int i = tid; i < TQ * KCAP; i += THREADS) lists[i] = 0;
    for (int i = tid; i < TQ; i += THREADS) locks[i] = 0;
    __syncthreads();
}
// write parts: the k kept keys of every pair go to out[probe rank][query][k]
template <int THREADS>
__device__ __forceinline__ void lvs_ivf_write_parts(const u64* lists, int KCAP, const int* slot_q, const int* slot_p, int npair, int k,
                                                    int nq, int tid, u64* out) {
    __syncthreads();
    for (int i = tid; i < npair * k; i += THREADS) {
        const int s = i / k, j = i - s * k;
        out[((long long)slot_p[s] * nq + slot_q[s]) * k + j] = lists[s * KCAP + j];
    }
}

// ---- host-side error plumbing ------------------------------------------------------------------------------
void lvs_set_error(const char* fmt, ...);
#define LVS_HIP_CHECK(expr)                                                                      \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            lvs_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return LVS_EDEVICE;                                                                  \
        }                                                                                        \
    } while (0)
#define LVS_REQUIRE(cond, ...)      \
    do {                            \
        if (!(cond)) {              \
            lvs_set_error(__VA_ARGS__); \
            return LVS_EINVAL;      \
        }                           \
    } while (0)

// Every workspace layout places its regions at multiples of 256 bytes from the base and reads them back as 64-bit keys, 64-bit
// atomics and 16-byte vectors: the base itself must sit on a multiple of 256 (include/lotus_hip.h; any hipMalloc'd pointer does).
#define LVS_WS_ALIGN 256
#define LVS_REQUIRE_WS_ALIGNED(ws) \
    LVS_REQUIRE(((uintptr_t)(ws) & (LVS_WS_ALIGN - 1)) == 0, "the workspace must be aligned to %d bytes", LVS_WS_ALIGN)

// Entry points launch on `stream`; make that stream's device current for the duration of the call (the caller may
// drive several GPUs from one process) and restore the previous one afterwards.
struct LvsDeviceGuard {
    int prev = -1;
    int dev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit LvsDeviceGuard(hipStream_t st) {
        err = hipGetDevice(&prev);
        dev = prev;
        if (err != hipSuccess || st == nullptr) return;
        hipDevice_t sd = 0;
        if (hipStreamGetDevice(st, &sd) != hipSuccess) {
            (void)hipGetLastError();
            return;  // legacy/default-stream handles: keep the current device
        }
        dev = (int)sd;
        if (dev != prev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~LvsDeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define LVS_DEVICE_GUARD(stream)                  \
    LvsDeviceGuard _lvs_guard((hipStream_t)(stream)); \
    LVS_HIP_CHECK(_lvs_guard.err)

// ---- zeroing scratch on the stream -------------------------------------------------------------------------
// A kernel of the library's own instead of hipMemsetAsync: in a captured graph hipMemsetAsync becomes a memset node, and from the
// graph's second launch on such a node has been seen (ROCm 7.0, gfx950) to leave part of the buffer non-zero for the kernel behind
// it - thresholds that reject every row, whole result lists empty (tests/test_gpu_stream_contract.py,
// profiles/stream_contract_check.md).  A kernel node replays like any launch.  p and bytes: multiples of 4.
template <int THREADS>
__global__ void lvs_zero_kernel(uint32_t* p, long long words) {
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < words; i += (long long)gridDim.x * THREADS) p[i] = 0u;
}
inline hipError_t lvs_zero_async(void* p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if ((bytes & 3) || ((uintptr_t)p & 3)) return hipErrorInvalidValue;
    const long long words = (long long)(bytes >> 2);
    const long long blocks = (words + 255) / 256;
    hipLaunchKernelGGL(lvs_zero_kernel<256>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, (uint32_t*)p, words);
    return hipGetLastError();
}

// ---- dynamic-LDS launches ----------------------------------------------------------------------------------
// More than 64 KB of dynamic LDS needs hipFuncSetAttribute(MaxDynamicSharedMemorySize), a per-device property of a kernel.
// lvs_arm_lds keeps one latch per kernel instantiation: which devices have the attribute (bit per device id) and for how
// many bytes, so it is set once per (kernel, device) and again only when a later call needs more.
#include <atomic>
struct LvsPerDeviceOnce {
    std::atomic<unsigned long long> mask{0};
    std::atomic<unsigned long long> bytes[64];
    bool done(int dev, size_t need) const {
        return dev >= 0 && dev < 64 && (mask.load(std::memory_order_acquire) >> dev & 1ull) &&
               bytes[dev].load(std::memory_order_relaxed) >= need;
    }
    void set(int dev, size_t have) {
        if (dev < 0 || dev >= 64) return;
        bytes[dev].store(have, std::memory_order_relaxed);
        mask.fetch_or(1ull << dev, std::memory_order_release);
    }
};
template <auto Kernel>
hipError_t lvs_arm_lds(size_t lds) {
    static LvsPerDeviceOnce attr;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || attr.done(dev, lds)) return e;
    e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) attr.set(dev, lds);
    return e;
}
template <auto Kernel, class... Args>
hipError_t lvs_launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args) {
    const hipError_t e = lvs_arm_lds<Kernel>(lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return hipGetLastError();
}
