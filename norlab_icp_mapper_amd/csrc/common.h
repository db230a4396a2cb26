// common.h -- internal declarations shared by the HIP translation units of libicpmi.so.
// Target: gfx950 (MI355X, CDNA4), wave64. Not a public header (the public one is include/icpmi.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <math.h>
#include <cstring>
#include <string>
#include <vector>
#include <unordered_map>
#include <mutex>
#include <map>
#include <cstdlib>
#include <shared_mutex>

#include "../../include/icpmi.h"

#define ICPMI_NV 32            // values of the minimiser's pair sums (27 of A / b or 16 of the point-to-point sums, sum w, pair count, force2D's b)
#define ICPMI_MAX_OUTLIER 8
#define ICPMI_MAX_SMOOTH 16
#define ICPMI_SEL_BINS 2048     // legacy 11/11/10 selection (stage entry point, chains with > 1 quantile filter)
// Fused selection (one quantile filter in the chain): two 16-bit radix levels of the d^2 bit pattern,
// each level a FINE histogram (65536 bins, direct device atomics: the values spread over hundreds of
// bins) plus a COARSE one over the top 8 bits of the digit (256 bins) that tells a consumer which 256
// fine bins to read.  Level 0's coarse histogram is hot (2-3 exponent values hold everything), so the
// NN workgroups aggregate it in LDS and flush into one of ICPMI_S2_COPIES privatised copies.
#ifndef ICPMI_S2_COPIES
#define ICPMI_S2_COPIES 8   // (r3: 32 -> 8: the level-0 scan of every selection workgroup sums the copies; +1 % on the k = 1 chains, 2 copies -3 %)
#endif
#define ICPMI_S2_C0 4096                                        // word offsets inside d_selhist (legacy bins first)
#define ICPMI_S2_F0 (ICPMI_S2_C0 + ICPMI_S2_COPIES * 256)
#ifndef ICPMI_S2_FCOPIES
#define ICPMI_S2_FCOPIES 1                                       // privatised copies of the level-0 FINE histogram
#endif
#define ICPMI_S2_C1 (ICPMI_S2_F0 + ICPMI_S2_FCOPIES * 65536)
#define ICPMI_S2_F1 (ICPMI_S2_C1 + 256)
// Pair-sum accumulators (r4), behind the histograms so that everything that clears the one clears the other: the ICPMI_NV sums of a
// registration's iteration as signed 64-bit FIXED-POINT device atomics -- integer additions commute, so the total does not depend on the
// order in which the pair-sum workgroups arrive, and what the solver reads is 32 values, not 64 KB of per-workgroup partials to be
// reduced in a fixed order.  A value v is held as two limbs, hi = rint(v 2^-16) and lo = rint((v - hi 2^16) 2^40): together 2^-40
// absolute resolution over +-2^78 with no range analysis, no carries between the limbs (they are summed independently and joined in
// double).  Headroom: |hi| <= 2^62 / adds by the range limit, and one contribution to lo is at most 2^15 x 2^40 = 2^55, so a copy that
// receives ICPMI_ACC_MAX_ADDS = 128 workgroup partials stays below 2^62 -- ONE bit inside int64, not more: loop.hip's acc_cap() clamps the
// number of pair-sum workgroups to ICPMI_ACC_MAX_ADDS x ICPMI_ACC_COPIES whatever ICPMI_ACC_BLOCKS asks for.
// ICPMI_ACC_COPIES privatised copies (workgroup b adds to copy b % COPIES),
// every (copy, value, limb) on its own 128-byte line: device atomics serialise per line.  (r4 kept two parities of them for the solve
// fused into the next NN launch; that path was removed in r5 -- DESIGN 13.3 -- and one set is left.)
#define ICPMI_ACC_COPIES 2   // (8 copies made every reader fetch 64 KB of padded lines -- 100 MB per NN launch once every workgroup reads them; 2: 128 atomics per line)
#define ICPMI_ACC_MAX_ADDS 128 // workgroup partials one copy may receive per iteration (limb headroom, see above)
#define ICPMI_ACC_PAD 16                                               // u64 per slot = one 128-byte line
#define ICPMI_ACC_U64 (ICPMI_ACC_COPIES * ICPMI_NV * 2 * ICPMI_ACC_PAD)   // 2048 u64 = 16 KiB
#define ICPMI_ACC_IDX(copy, i, limb) ((((copy) * ICPMI_NV + (i)) * 2 + (limb)) * ICPMI_ACC_PAD)
#define ICPMI_ACC_FLAG (ICPMI_ACC_IDX(0, 0, 0) + 8)                    // a non-finite partial was met (NaN must reach the solver: ICPMI_ERR_NAN)
#define ICPMI_S2_ACC (ICPMI_S2_F1 + 65536)                             // u32 word offset of the accumulators (128-byte aligned)
// (r5) Speculative level 0 for the k > 1 loop (nnk_wg_kernel builds it, select.hip: win_lookup reads it).  The 16-bit prefix the selection
// picks moves by a fraction of a bin from one iteration to the next once the registration settles, and the stand-alone level-0 builder
// costs 10.7 us per iteration at knn 6 (116 k device atomics: DESIGN 11.6, 12.8).  So the NN kernel counts its own k x 64 distances into
// ICPMI_WIN_BINS bins around the PREVIOUS iteration's prefix plus "below" and "above" -- nine counts, reduced inside the wave, three
// 64-bit atomics per workgroup (three 21-bit fields each: the host enables the window only below 2^21 matches, so no field can carry) --
// and when the selected rank falls inside the window the builder launch has nothing to do.  A miss (the first iterations, a limit that
// jumps) is the full histogram as before; the counts are exact either way, so the selected element is the same bit pattern.
// Every (copy, word) on its own 128-byte line; the header word holds (lowest window prefix + 1), 0 = no window this iteration.
#define ICPMI_WIN_BINS 7
#ifndef ICPMI_WIN_COPIES
#define ICPMI_WIN_COPIES 8
#endif
#define ICPMI_WIN_PAD 16                                                  // u64 per slot = one 128-byte line
#define ICPMI_WIN_HDR (ICPMI_WIN_COPIES * 3 * ICPMI_WIN_PAD)              // u64 index of the header
#define ICPMI_WIN_U64 (ICPMI_WIN_HDR + ICPMI_WIN_PAD)
#define ICPMI_WIN_MAX_COUNT (1ll << 21)
#define ICPMI_S2_WIN (ICPMI_S2_ACC + 2 * ICPMI_ACC_U64)                   // u32 word offset of the window (128-byte aligned)
#define ICPMI_SELHIST_WORDS (ICPMI_S2_WIN + 2 * ICPMI_WIN_U64)
// Device atomics serialise per cache line, and neighbouring fine bins are hot together: bin b of a fine
// histogram lives at word ((b & 255) << 8) | (b >> 8), i.e. consecutive bins are 1 KiB apart.
#define ICPMI_S2_FIDX(b) ((((b) & 255u) << 8) | ((b) >> 8))

#define ICPMI_MAX_K 32

// Once-touched streams (queries, per-query loop state, matches) with the non-temporal cache policy (`nt`): -DICPMI_NT_STREAMS.  r5
// measurement: an XCD's L2 does not keep ANY line across a kernel boundary on this part (the second of two back-to-back NN
// launches fetches the same 20.6 MB past the L2 as the first), so there is no map slice for these streams to push out between launches;
// inside a launch the hint changed nothing measurable.  Kept as a switch; plain loads / stores by default.
#ifdef __HIPCC__
// ---- exchanges between the lanes of a wave, in registers.  PRECONDITION of everything in this block: every lane of the wave is active at
// the call (a DPP / permlane read of an inactive lane does not give that lane's value) ----
// inclusive prefix sum over the 64 lanes of a wave (DPP: shifts within rows of 16 lanes, then the row totals broadcast into the following
// rows)
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1, 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31 -> rows 2, 3
    return v;
}
// value of lane (lane ^ J), without the LDS crossbar: DPP quad permutes / row shifts / row rotate inside a row of 16 lanes, gfx950's
// v_permlane16_swap / v_permlane32_swap across rows (a sort written with __shfl_xor is 42 ds_bpermute_b32 round trips, one behind the other)
template <int J>
__device__ __forceinline__ unsigned lane_xor(unsigned v)
{
    static_assert(J == 1 || J == 2 || J == 4 || J == 8 || J == 16 || J == 32, "one bit of the lane index");
    const int x = (int)v;
    if constexpr (J == 1) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);      // quad_perm [1, 0, 3, 2]
    else if constexpr (J == 2) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false); // quad_perm [2, 3, 0, 1]
    else if constexpr (J == 4) {
        const int t = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);                            // row_shl:4 into banks 0, 2
        return (unsigned)__builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);                         // row_shr:4 into banks 1, 3
    } else if constexpr (J == 8) return (unsigned)__builtin_amdgcn_update_dpp(x, x, 0x128, 0xF, 0xF, false); // row_ror:8
    else if constexpr (J == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); // r[0]: odd rows <- even rows; r[1]: even rows <- odd rows
        return (threadIdx.x & 16) ? r[0] : r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (threadIdx.x & 32) ? r[0] : r[1];
    }
}
template <int J>
__device__ __forceinline__ unsigned long long lane_xor64(unsigned long long v)
{
    return ((unsigned long long)lane_xor<J>((unsigned)(v >> 32)) << 32) | (unsigned long long)lane_xor<J>((unsigned)v);
}
template <int J> // a double travels as its two 32-bit halves: the bits arrive as they left
__device__ __forceinline__ double lane_xor(double v)
{
    return __longlong_as_double((long long)lane_xor64<J>((unsigned long long)__double_as_longlong(v)));
}
// the same with the partner's bit as a value: for unrolled loops over m = 1, 2, .. 32 (m is a constant in every unrolled body, and only
// that body's exchange is left of the switch)
__device__ __forceinline__ double lane_xor_bit(double v, int m)
{
    switch (m) {
    case 1: return lane_xor<1>(v);
    case 2: return lane_xor<2>(v);
    case 4: return lane_xor<4>(v);
    case 8: return lane_xor<8>(v);
    case 16: return lane_xor<16>(v);
    default: return lane_xor<32>(v);
    }
}

// Rank lookups in the fused selection's histograms, shared by the kernels that build them (select.hip) and the consumers that resolve the
// last level (loop.hip: accumulate_kernel, res_pairs_kernel).
// All 256 threads call with one bin count `v` each (bin = threadIdx.x).  Finds the bin holding element
// `rank` (0-based, ascending); when from_quantile, rank = (unsigned)(float(total) * quantile) like
// getDistsQuantile.  Results are uniform across the block.
// REG_SCAN: the wave's prefix sums in registers (wave_incl_scan); false: the __shfl_up scan, for a caller that spills more with the former
// (integer adds: the same sums either way).
template <bool REG_SCAN = true>
__device__ __forceinline__ void block_find_rank256(unsigned v, bool from_quantile, float quantile, unsigned rank_in,
                                                   unsigned* sh /* >= 16 words */, unsigned& bin, unsigned& rank_rem, unsigned& total)
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    unsigned incl = v;
    if constexpr (REG_SCAN) incl = wave_incl_scan(v);
    else {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
    }
    if (lane == 63) sh[wv] = incl;
    __syncthreads();
    const unsigned w0 = sh[0], w1 = sh[1], w2 = sh[2], w3 = sh[3];
    total = w0 + w1 + w2 + w3;
    incl += wv == 0 ? 0u : (wv == 1 ? w0 : (wv == 2 ? w0 + w1 : w0 + w1 + w2));
    const unsigned excl = incl - v;
    unsigned rank = rank_in;
    if (from_quantile) {
        if (total == 0) rank = 0;
        else if (quantile == 1.0f) rank = total - 1;
        else {
            rank = (unsigned)((float)total * quantile);
            if (rank > total - 1) rank = total - 1;
        }
    }
    if (total != 0 && rank >= excl && rank < incl) { sh[8] = (unsigned)t; sh[9] = rank - excl; }
    __syncthreads();
    bin = sh[8];
    rank_rem = sh[9];
    __syncthreads(); // (stays: in a 1024-thread workgroup the next call's sh[wv] reaches words 8 and 9 in front of its first barrier)
}

// two-tier lookup: coarse bin from `coarse_v` (this thread's coarse count), then the fine bin under it
template <int FCOPIES, bool REG_SCAN = true>
__device__ __forceinline__ void block_find_rank_2tier(unsigned coarse_v, const unsigned* __restrict__ fine, bool from_quantile,
                                                      float quantile, unsigned rank_in, unsigned* sh, unsigned& bin16,
                                                      unsigned& rank_rem, unsigned& total)
{
    unsigned cb, rem, tot2;
    block_find_rank256<REG_SCAN>(coarse_v, from_quantile, quantile, rank_in, sh, cb, rem, total);
    if (total == 0) { bin16 = 0; rank_rem = 0; return; }
    unsigned fv = 0;
    if (threadIdx.x < 256) { // (workgroups wider than 256 threads: the extra waves carry empty bins through the scan)
#pragma unroll
        for (int cpy = 0; cpy < FCOPIES; ++cpy) fv += fine[cpy * 65536 + ICPMI_S2_FIDX(cb * 256 + threadIdx.x)];
    }
    unsigned fb;
    block_find_rank256<REG_SCAN>(fv, false, 0.f, rem, sh, fb, rank_rem, tot2);
    bin16 = (cb << 8) | fb;
}

typedef float icpmi_vf4 __attribute__((ext_vector_type(4)));
#ifdef ICPMI_NT_STREAMS
__device__ __forceinline__ float4 ld_stream(const float4* p) { const icpmi_vf4 v = __builtin_nontemporal_load(reinterpret_cast<const icpmi_vf4*>(p)); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ float ld_stream(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ int ld_stream(const int* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_stream(float4* p, float4 v) { icpmi_vf4 w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w; __builtin_nontemporal_store(w, reinterpret_cast<icpmi_vf4*>(p)); }
__device__ __forceinline__ void st_stream(float* p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void st_stream(int* p, int v) { __builtin_nontemporal_store(v, p); }
#else
template <class T> __device__ __forceinline__ T ld_stream(const T* p) { return *p; }
template <class T> __device__ __forceinline__ void st_stream(T* p, T v) { *p = v; }
#endif
// Write-through stores (`sc1`) for what a loop kernel hands to the NEXT kernel: the bytes leave the XCD's L2 as the store is issued and leave
// no dirty line behind, so the write-back of the eight L2s at the kernel boundary finds nothing of them (a plain or `nt` store keeps the
// line, dirty, until that write-back).  Nothing is ordered by them: the kernel boundary orders producer and consumer as before.  4 bytes: a
// relaxed agent-scope atomic store (global_store_dword ... sc1).  16 bytes: ONE global_store_dwordx4 ... sc1 -- no builtin gives that
// instruction through a plain pointer, so it is one line of assembly; the s_nop keeps the compiler's next instruction off the data
// registers until the store has read them.  Dword-wide write-through stores are one fabric write each (about six times the 16-byte cost
// per byte): for wide streams and clears only, unless measured.
__device__ __forceinline__ void st_wt(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_wt(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_wt(uint4* p, uint4 v)
{
    typedef unsigned icpmi_vu4 __attribute__((ext_vector_type(4)));
    icpmi_vu4 w; w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(w) : "memory");
}
__device__ __forceinline__ void st_wt(float4* p, float4 v)
{
    st_wt(reinterpret_cast<uint4*>(p), make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)));
}
// The sites, one compile-time switch each (0 = the plain store the site had).  The defaults are what the alternating A/B of DESIGN 4.2
// (profiles/store_policy_bench.json, 12 rounds of the headline) left on: the clears alone +1.5 %, the clears with all three result streams
// of the k = 1 matcher +2.9 %; the result streams WITHOUT the clears stay inside the parent's run-to-run range, and so does everything the
// head of a registration writes (qfirst_kernel, qpass_kernel: built, measured, taken out again).
//   ICPMI_WT_MATCH     nn1_wg_kernel's matched points (match_pt, 16 bytes per query)
//   ICPMI_WT_RESULT    nn1_wg_kernel's dword-wide result streams (out_sidx, out_d2)
//   ICPMI_WT_RESULT_K  ... those of nnk_ml_kernel and nnk_wg_kernel (k dwords per query and stream)
//   ICPMI_WT_CLEAR     the per-iteration histogram clears (nn1_wg_kernel, accumulate_kernel, sel2_hist0_kernel), as 16-byte zero stores
//                      from a quarter of the threads
#ifndef ICPMI_WT_MATCH
#define ICPMI_WT_MATCH 1
#endif
#ifndef ICPMI_WT_RESULT
#define ICPMI_WT_RESULT 1
#endif
#ifndef ICPMI_WT_RESULT_K
#define ICPMI_WT_RESULT_K 0
#endif
#ifndef ICPMI_WT_CLEAR
#define ICPMI_WT_CLEAR 1
#endif
template <int WT, bool STREAM = true, class T> __device__ __forceinline__ void st_policy(T* p, T v) // STREAM: a st_stream site when not written through
{
    if constexpr (WT != 0) st_wt(p, v);
    else if constexpr (STREAM) st_stream(p, v);
    else *p = v;
}
// ICPMI_WT_CLEAR: `words` zeroed words at p (16-byte aligned, words % 4 == 0) by the threads gtid, gtid + stride, ... of a launch, 16 bytes a
// store (2: the same width with plain stores, for the A/B of width against policy)
__device__ __forceinline__ void clear_words_wt(unsigned* p, int words, int64_t gtid, int64_t stride)
{
    for (int64_t i = gtid; i < words / 4; i += stride) st_policy<(ICPMI_WT_CLEAR == 1), false>(reinterpret_cast<uint4*>(p) + i, make_uint4(0u, 0u, 0u, 0u));
}
static_assert(ICPMI_S2_C0 % 4 == 0 && ICPMI_S2_C1 % 4 == 0 && ICPMI_S2_WIN % 4 == 0 && ICPMI_SELHIST_WORDS % 4 == 0 && (2 * ICPMI_WIN_U64) % 4 == 0,
              "the cleared regions of d_selhist start and end on 16 bytes");

// ---- runs of equal keys inside a wave become ONE atomic per run (counting sorts: map_build.hip, the DynamicPoints bucket grid) ----
struct WaveRun { bool head; int rank; int len; int head_lane; };
__device__ __forceinline__ WaveRun wave_run(unsigned key, bool valid)
{
    const int lane = threadIdx.x & 63;
    const unsigned prev = (unsigned)__shfl_up((int)key, 1, 64);
    const bool pvalid = __shfl_up((int)valid, 1, 64) != 0;
    const bool head = valid && (lane == 0 || !pvalid || prev != key);
    const unsigned long long heads = __ballot(head);
    const unsigned long long valids = __ballot(valid);
    WaveRun r;
    r.head = head;
    const unsigned long long below = heads & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
    r.head_lane = below ? 63 - __clzll((long long)below) : lane;
    r.rank = lane - r.head_lane;
    const unsigned long long above = (lane == 63) ? 0ull : (heads & ~((2ull << lane) - 1ull));
    const int nvalid = __popcll(valids); // valid lanes are a prefix of the wave
    const int end = above ? (__ffsll((long long)above) - 1) : nvalid;
    r.len = end - r.head_lane;
    return r;
}
// ---- the flagged lanes of a wave append to a list with ONE atomic on its counter (by lane 0: every lane of the wave must be active);
// returns the slot of a flagged lane (flagged lanes in lane order), nothing of use for the others ----
__device__ __forceinline__ unsigned wave_append(unsigned* counter, bool flag)
{
    const unsigned long long bal = __ballot(flag);
    if (!bal) return 0u;
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(counter, (unsigned)__popcll(bal));
    base = (unsigned)__builtin_amdgcn_readlane((int)base, 0);
    return base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
}
// (the prefix sum over a wave's lanes, wave_incl_scan, stands with the lane exchanges above)
#endif

// ------------------------------------------------------------------------------------------------
// NN grid (built by set_map on the centred map).  Dense uniform grid; cells are x-fastest so the
// three x-neighbours of a cell row are one contiguous run of the cell-sorted point array.
// ------------------------------------------------------------------------------------------------
struct GridParams {
    float ox, oy, oz;      // min corner (centred frame)
    float cell, inv_cell;  // cell edge and its reciprocal
    float slack;           // conservative distance slack for prune / termination tests
    int   nx, ny, nz;
    int   ncells;
};

// Pyramid of grids over the same bounding box: level l has cell edge cell0 * 2^l and its own
// cell-sorted copy of the map.  A query that cannot be decided inside the 3x3x3 block of level l
// (best distance beyond its margin) repeats the identical 27-cell search one level up, where the
// block is twice as wide -- no ring bookkeeping, and always one contiguous x-run per (y, z) row.
#define ICPMI_MAXLEV 8
struct GridLevels {
    int nlev;
    GridParams g[ICPMI_MAXLEV];
    const float4* pts[ICPMI_MAXLEV];    // cell-sorted points of the level: xyz centred, w = original index bits
    const unsigned* cs[ICPMI_MAXLEV];   // cell starts of the level (ncells + 1)
    const unsigned* pos0[ICPMI_MAXLEV]; // level position -> level-0 position (nullptr for level 0)
};

// One level of the pyramid as the NN kernels read it: c->d_lvl_tab holds ICPMI_MAXLEV of these (upload_level_table, map_build.hip), a kernel
// copies them into LDS as four uint4 words per level and reads them through level_grid / level_cs / level_pts / level_pos0 below.
struct LevelRow {
    float ox, oy, oz, cell;       // word 0
    float inv_cell, slack;        // word 1
    int nx, ny;
    int nz, ncells;               // word 2
    const float4* pts;
    const unsigned* cs;           // word 3
    const unsigned* pos0;
};
static_assert(sizeof(LevelRow) == 64 && offsetof(LevelRow, inv_cell) == 16 && offsetof(LevelRow, nz) == 32 && offsetof(LevelRow, pts) == 40 &&
              offsetof(LevelRow, cs) == 48 && offsetof(LevelRow, pos0) == 56, "four uint4 words, pointers in the halves the readers take them from");

// Batched registration (icpmi_register_batch_dev): B independent readings against the same map go through ONE launch
// of every kernel of the loop, blockIdx.y = reading.  Per-reading arrays are slices of one allocation (slice b starts
// at b * qstride elements; selection histograms, pair-sum partials and the IcpState array have their own fixed
// strides).  A single registration is the batch of one (blockIdx.y == 0, every offset 0): the SAME kernels serve
// both, so a reading registers to the same bits alone or in a batch.
#define ICPMI_MAX_BATCH 16
struct BatchArgs {
    int nscan;
    int qstride;                 // elements between the per-reading slices of the per-query arrays
    int n[ICPMI_MAX_BATCH];      // points of every reading
};
struct BatchSrc { const float4* p[ICPMI_MAX_BATCH]; }; // the readings as handed in (device pointers)
// maxDist -> the squared accept radius the matcher kernels compare d2 with: THE expression for KDTreeMatcher's maxDist and for every entry
// of a KDTreeVarDistMatcher row alike (a constant row gives the bits of maxDist)
static inline float squared_radius(float r) { return std::isinf(r) ? INFINITY : r * r; }
static inline BatchArgs batch_of_one(int64_t n) { BatchArgs b; memset(&b, 0, sizeof b); b.nscan = 1; b.n[0] = (int)n; return b; }

// What the pair-sum kernel adds per pair (loop.hip: accumulate_kernel's template parameter).  make_loop_cfg chooses it; LoopCfg::minimizer
// beside it stays the kind of normal equations every kernel BEHIND the pair sums sees: the last four all fill the point-to-plane slots.
enum PairModel { PAIR_IDENTITY, PAIR_POINT_TO_POINT, PAIR_POINT_TO_PLANE, PAIR_PLANE_TO_PLANE, PAIR_SYMMETRIC, PAIR_INTENSITY };
// ... the models that read the map's normals (and fill the 27 point-to-plane slots)
constexpr bool pair_reads_map_normals(PairModel pm)
{
    return pm == PAIR_POINT_TO_PLANE || pm == PAIR_PLANE_TO_PLANE || pm == PAIR_SYMMETRIC || pm == PAIR_INTENSITY;
}

// Device-side description of the ICP chain for one registration (passed by value to kernels).
struct LoopCfg {
    int   k;
    float max_dist;        // un-squared; +inf allowed
    float maxr2;           // max_dist^2 (+inf allowed)
    float inv1e, err2;     // KDTreeMatcher's epsilon when icpmi_config::epsilon_approx asks for it: 1 / (1 + epsilon) and (1 + epsilon)^2; both 1 otherwise
    int   ring_max;        // rings searched on the grid before a query goes to the brute pass
    int   minimizer;
    int   n_out;
    int   out_type[ICPMI_MAX_OUTLIER];
    float out_param[ICPMI_MAX_OUTLIER];
    int   out_iparam[ICPMI_MAX_OUTLIER];
    float out_param2[ICPMI_MAX_OUTLIER];
    float out_param3[ICPMI_MAX_OUTLIER];
    int   ext;             // GenericDescriptor / Robust in the chain: the pair-sum kernel's EXT variant
    int   force_4dof;
    int   force_2d;        // (routes the pair sums through the EXT variant: three more sums, b of the 2-D residual)
    int   is_2d;           // planar clouds: point-to-point solves the in-plane rotation in closed form
    int   max_iter;
    int   use_diff;
    float min_rot, min_trans;
    int   smooth;
    int   use_bound;
    float max_rot, max_trans;
    int   has_read_normals;
    int   sensor_noise;    // the reading carries simpleSensorNoise + normals: getOverlap() is the sensor-noise count (loop.hip: overlap pass)
    const float* read_scalar; // GenericDescriptorOutlierFilter{source: reading}: that descriptor of the reading, caller's order (device)
    // degeneracy-aware point-to-plane solve (icpmi_config::degeneracy_threshold; solve.h: degen_*): 0 off, ICPMI_DG_REPORT, ICPMI_DG_CONSTRAIN
    int   degen;
    float degen_thr;          // |degeneracy_threshold|
    double* degen_blk;        // the handle's side block (layout below), null when off
    // the pair sums' model and what it alone reads; each field is 0 unless pair_model owns it (loop_sig hashes the bytes: a change of model,
    // epsilon or weight misses a cached graph)
    int   pair_model;         // PairModel
    float plane_eps;          // PAIR_PLANE_TO_PLANE: epsilon of the covariances C(n) = I - (1 - eps) n n^T, in (0, 1]
    float intensity_w;        // PAIR_INTENSITY: the photometric weight 1 - lambda, in (0, 1)
    const float4* map_gi;     // ... the map's (g.x, g.y, g.z, I) per point, in the index's order (null: no current channel)
    const float* read_intensity; // ... the intensity row of THIS reading, caller's order (api.hip: intensity_setup)
};
// slot of the chain's Trimmed / Median / VarTrimmed filter (the last of them: the one whose limit a call reports), or -1.  Upstream, a
// chain with one throws "no outlier to filter" on an empty reading where any other throws "no point to minimize".
static inline int quantile_slot(const LoopCfg& lc)
{
    int slot = -1;
    for (int f = 0; f < lc.n_out; ++f)
        if (lc.out_type[f] == ICPMI_OUT_TRIMMEDDIST || lc.out_type[f] == ICPMI_OUT_MEDIANDIST || lc.out_type[f] == ICPMI_OUT_VARTRIMMEDDIST) slot = f;
    return slot;
}
static inline bool chain_has_quantile(const LoopCfg& lc) { return quantile_slot(lc) >= 0; }
// index of the single quantile-type filter of the chain, or -1 (none) / -2 (more than one)
static inline int fused_filter_slot(const LoopCfg& lc)
{
    int slot = -1;
    for (int f = 0; f < lc.n_out; ++f)
        if (lc.out_type[f] == ICPMI_OUT_TRIMMEDDIST || lc.out_type[f] == ICPMI_OUT_MEDIANDIST) slot = slot == -1 ? f : -2;
    return slot;
}

// The matcher's output as the passes that walk it see it (loop.hip: pair_view fills it on the host, walk_pairs reads it on the device): slot
// e of the n * k belongs to query e / k of `reading`; `reading`, sidx, d2 (and match_pt, the matched points the k = 1 matcher keeps) share one
// order -- the caller's, or, qindex != nullptr, the tile-sorted one, where qindex maps a query back to the caller's index (read_normals and
// the reading's other descriptors stay in the caller's order).  A null pointer = the chain has no such array.
struct PairView {
    const float4* __restrict__ reading;
    const int*    __restrict__ qindex;
    const int*    __restrict__ sidx;
    const float*  __restrict__ d2;
    const float4* __restrict__ match_pt;
    const float4* __restrict__ map;          // cell-sorted map points, w = original index bits
    const float4* __restrict__ ref_normals;  // of the map, same order
    const float4* __restrict__ read_normals;
    const float*  __restrict__ ref_scalar;   // the map's tracked scalar descriptor, by ORIGINAL index (EXT chains)
};

// the side block of the degeneracy-aware solve (icpmi_ctx::d_degen), in doubles
#define ICPMI_DG_REPORT 1
#define ICPMI_DG_CONSTRAIN 2
#define ICPMI_DG_C0 0        // c0 (3) and L: the reading's statistics, once per registration (loop.hip: degen_stats_*)
#define ICPMI_DG_SUMS 8      // tot[0..28] of the last counted iteration, as its solve read them
#define ICPMI_DG_T 40        // the 16 floats of T_iter that iteration's pairs were formed under
#define ICPMI_DG_ITER 56     // the iteration's number (1 = the first)
#define ICPMI_DG_OUT 64      // icpmi_localizability as degen_report_kernel leaves it (pivot still in the centred frame)
#define ICPMI_DG_PART 128    // ICPMI_DG_NB x 4 partial sums of the statistics
#define ICPMI_DG_NB 64
#define ICPMI_DG_DOUBLES (ICPMI_DG_PART + 4 * ICPMI_DG_NB)
static_assert(sizeof(icpmi_localizability) <= (ICPMI_DG_PART - ICPMI_DG_OUT) * sizeof(double), "the report fits its slot of the side block");

// Device-resident loop state (one per handle).  Everything the iteration needs between kernels
// lives here so that the loop never synchronises with the host.
// The words the per-iteration kernels READ sit together at the front (LoopHdr: 42 dwords on two adjacent 128-byte lines), so that a
// kernel fetches them with ONE load instruction of one wave (hdr_load below: lane l takes dword l) issued next to its first data loads,
// instead of one dependent miss per field on five different lines.  Everything a kernel only writes, or only the solve's checkers and
// the host read, stays behind the header.
struct alignas(128) LoopHdr {
    float T_iter[16];
    int   iter;
    int   done;
    int   error;           // icpmi_status (0 = ok)
    int   counter;
    int   hist_n;          // number of poses pushed to the differential checker
    unsigned seq;          // registration sequence number (tag of the progress word, see icpmi_ctx::h_progress)
    unsigned hard_count;
    unsigned n_valid;
    unsigned sel_prefix_l[3];  // fused selection: one slot per radix level (written by level L,
    unsigned sel_rank_l[3];    // read by level L + 1 -- never both in one kernel)
    float robust_scale;    // RobustOutlierFilter::scale, kept between iterations (nbIterationForScale)
    unsigned vox_level;    // scheduled VoxelMatcher handles only (voxel.hip sets, reads and raises it; nothing else touches the word): the current level
    float limits[ICPMI_MAX_OUTLIER];
    // r6: device clock at which the last NN launch's first workgroup started (0: no interval open), see t_nn_sum below
    unsigned long long t_nn_begin;
};
static_assert(sizeof(LoopHdr) == 256 && alignof(LoopHdr) == 128, "the loop header is two 128-byte lines: one dword per lane of a wave");
#define ICPMI_HDR_W(field) ((int)(offsetof(LoopHdr, field) / 4))   // dword index of a header field = the lane that holds it after hdr_load

#define ICPMI_NN_DEFER_WGS_DEFAULT 160 // helper workgroups of a k = 1 loop launch (a multiple of 8; with the 1 568 home workgroups of 100 k queries all 1 792 resident slots hold up to 224)
#define ICPMI_NN_DEFER_WGS_MAX 224
#define ICPMI_TL_LAUNCHES 24   // -DICPMI_NN_TIMING: NN launches of a registration whose workgroup timeline is kept (nn.hip)
struct IcpState : LoopHdr {
    int   stop_reason;
    double hq[(ICPMI_MAX_SMOOTH + 1) * 4];
    double ht[(ICPMI_MAX_SMOOTH + 1) * 3];
    double hrot[ICPMI_MAX_SMOOTH + 1];   // |angular distance| and translation distance between pose slot i and the pose before it
    double htr[ICPMI_MAX_SMOOTH + 1];
    double init_q[4];
    // quantile selection
    unsigned sel_prefix;
    unsigned sel_rank;
    unsigned vt_valid;     // VarTrimmedDist: number of valid matches of this iteration (counted by vt_keys_kernel, cleared by vt_pick_kernel)
    float vt_ratio;        // ... and the ratio optimizeInlierRatio picked (diagnostic)
    float robust_med;      // RobustOutlierFilter{mad}: median of the finite d2 of this iteration
    // statistics of the last iteration
    long long pairs;
    double wsum;
    unsigned ticket;             // workgroups of the pair-sum kernel that have published their partials (last one solves)
    unsigned long long hard_total;
    unsigned long long dbg[24];  // diagnostics: NN phase cycles with -DICPMI_NN_TIMING (scripts/nn_phase.py), [20]/[21] serial solve cycles / calls
    float T_prev[16];            // T_iter BEFORE the last minimisation: the pose the last counted iteration's pairs were formed under
    // result
    float T_out[16];
    // r5: device clocks (wall_clock64, 100 MHz) of the first kernel of the registration's head and of the solve that stopped the loop:
    // stats->loop_ms without a HIP event to wait for (loop_run's fast finish).  t_done == 0: the loop was not stopped by a solve.
    unsigned long long t_start, t_done;
    // r6: device-clock interval of every NN launch, summed over the registration: opened by the NN kernel's first workgroup (t_nn_begin),
    // closed by the first workgroup of whatever kernel runs next (so one kernel boundary is inside) -- icpmi_stats::nn_ms_avg of a loop that
    // is NOT in profile mode, i.e. bench.py's roofline duration taken from the timed graph replay itself
    unsigned long long t_nn_sum;
    unsigned nn_count, pad_nn;
    // k = 1 matcher, deferral of far-seeded queries (nn.hip: nn1_wg_kernel): the NN launch of iteration i serves list i % 3, appends to list
    // (i + 1) % 3 and zeroes the count of list (i + 2) % 3, which nobody touches in that launch.  A count may exceed the lists' capacity
    // (readers clamp it).  defer_served / defer_overflow: queries the helper workgroups ran / heavy queries that found their list full,
    // summed over the registration (icpmi_debug_counters 10 / 11).  Behind everything else: no other field moves.
    unsigned defer_count[3];
    unsigned defer_served, defer_overflow, pad_defer;
#ifdef ICPMI_NN_TIMING
    // timing builds only (scripts/nn_wg_timeline.py): the open and the close stamp of every NN launch of the registration, by launch number
    unsigned long long tl_open[ICPMI_TL_LAUNCHES], tl_close[ICPMI_TL_LAUNCHES];
#endif
};

#ifdef __HIPCC__
// One trip for the loop header: every lane of the calling wave (all 64 active) loads the dword of its lane number; a field is then a
// readlane of that register (uniform, no memory access).  Issue it in front of the kernel's first data loads and join the two at one point.
__device__ __forceinline__ unsigned hdr_load(const IcpState* st) { return reinterpret_cast<const unsigned*>(st)[threadIdx.x & 63]; }
struct HdrView {
    unsigned w; // lane l: dword l of the header
    __device__ __forceinline__ unsigned u(int i) const { return (unsigned)__builtin_amdgcn_readlane((int)w, i); }
    __device__ __forceinline__ int i(int idx) const { return __builtin_amdgcn_readlane((int)w, idx); }
    __device__ __forceinline__ float f(int idx) const { return __int_as_float(__builtin_amdgcn_readlane((int)w, idx)); }
    __device__ __forceinline__ unsigned long long u64(int idx) const { return (unsigned long long)u(idx) | ((unsigned long long)u(idx + 1) << 32); }
};
__device__ __forceinline__ void nn_stamp_open(IcpState* st) { st->t_nn_begin = (unsigned long long)wall_clock64(); }
// close the interval the last NN launch opened.  `b` = t_nn_begin as the caller already holds it (from its header read): no load at all,
// the sum and the count go out as no-return atomics.  Several kernels may follow one NN launch: whoever finds the interval open closes it.
__device__ __forceinline__ void nn_stamp_close(IcpState* st, unsigned long long b)
{
    if (b) {
#ifdef ICPMI_NN_TIMING
        const unsigned long long now = (unsigned long long)wall_clock64();
        atomicAdd(&st->t_nn_sum, now - b);
        const unsigned launch = atomicAdd(&st->nn_count, 1u);
        if (launch < ICPMI_TL_LAUNCHES) { st->tl_open[launch] = b; st->tl_close[launch] = now; }
#else
        atomicAdd(&st->t_nn_sum, (unsigned long long)wall_clock64() - b);
        atomicAdd(&st->nn_count, 1u);
#endif
        st->t_nn_begin = 0;
    }
}
__device__ __forceinline__ void nn_stamp_close(IcpState* st) { nn_stamp_close(st, st->t_nn_begin); }
#endif


// ------------------------------------------------------------------------------------------------
// Device memory through a process-wide block cache (r5).  hipFree unmaps the block behind a device-wide synchronisation and hipMalloc
// maps a new one (~0.1 - 0.3 ms a pair at the sizes of a map's arrays); a mapper grows ~20 arrays by doubling while its map grows, every
// operator call holds a few temporaries, and a replay that builds a fresh mapper pays all of it again (BASELINE config 4: the first two of
// 14 scans were 14 of 37 ms).  dev_free keeps the block (after the same device-wide synchronisation hipFree implies: nothing in flight
// can still touch it), dev_malloc hands out the smallest cached block of at least the size asked for and at most twice that + 1 MiB.
// ICPMI_ALLOC_CACHE_MB (default 1024; 0: plain hipMalloc / hipFree) bounds what is kept; the largest blocks go first.  Blocks are cached per
// device.  Cached blocks go back to the runtime at exactly two points: icpmi_trim_cache(), and dev_malloc's out-of-memory path.  Destroying
// handles -- the last one of the process included -- releases nothing (icpmi_destroy only keeps the count of live handles): a process holds up
// to ICPMI_ALLOC_CACHE_MB of HBM after its mappers are gone until it calls icpmi_trim_cache().
// ------------------------------------------------------------------------------------------------
// A device-wide synchronisation and a stream capture in ANOTHER thread do not mix on this runtime (scripts/r5/capture_threads.hip, ROCm 7:
// hipDeviceSynchronize fails with "operation not permitted when stream is capturing" AND invalidates the other thread's thread-local capture;
// so does a synchronous hipMemcpy / hipMemset on the legacy stream; hipMalloc / hipFree / hipStreamCreate / hipHostMalloc / launches do not).
// One handle per thread is the contract of icpmi.h -- a mapper's update thread next to its registration thread (Mapper.cpp:274-288) is exactly
// that -- so: a thread that captures holds this gate shared from BeginCapture to EndCapture (host-side work only), dev_free takes it exclusive
// around its hipDeviceSynchronize, and the library makes no synchronous legacy-stream call outside diagnostics.
inline std::shared_mutex& capture_gate() { static std::shared_mutex* m = new std::shared_mutex; return *m; } // (never destroyed: see dev_block_cache)
struct CaptureGate {
    CaptureGate() { capture_gate().lock_shared(); }
    ~CaptureGate() { capture_gate().unlock_shared(); }
    CaptureGate(const CaptureGate&) = delete;
    CaptureGate& operator=(const CaptureGate&) = delete;
};

// One cached loop graph (loop.hip: capture_loop_graph): valid for the registrations whose signature is `sig`.  `sorted` is the loop state
// order it leaves (NnOutcome::out_sorted of its last launch, as captured); a head graph of a checked loop also keeps its length and an LRU stamp.
struct LoopGraph {
    hipGraphExec_t exec = nullptr; uint64_t sig = 0; int uses = 0; bool sorted = false;
    int len = 0; unsigned long used = 0;
    bool holds(uint64_t s) const { return exec && sig == s; }
    void reset() { if (exec) hipGraphExecDestroy(exec); *this = LoopGraph(); }
};
// every graph of a handle's loops: one fixed-count registration, one batched registration, a checked loop's SEGMENT graphs ([0] = head + the
// first S iterations, [1] = S further iterations, replayed while the progress word says the loop is still running) and (r5) head graphs of
// OTHER lengths (head + L iterations, L = the iteration count of the handle's previous checked registration: a mapper's registrations stop
// after about the same number of iterations scan after scan, and a head graph of exactly that length has no dead iterations)
struct LoopGraphs {
    LoopGraph fixed, batch, seg[2], heads[4];
    unsigned long clock = 0;
    void reset() { fixed.reset(); batch.reset(); for (LoopGraph& g : seg) g.reset(); for (LoopGraph& g : heads) g.reset(); }
};

struct DevBlockCache {
    struct Live { size_t bytes; int dev; };
    std::mutex mu;
    std::unordered_map<void*, Live> live;                  // every block handed out -> its true size and the device it was mapped on
    std::map<int, std::multimap<size_t, void*>> idle_of;   // cached blocks by size, PER DEVICE (r6, ADVICE r5: icpmi_config::device puts several GPUs in one process)
    size_t idle_bytes = 0, limit = 0;
    long handles = 0;                                      // live top-level handles (icpmi_create / icpmi_destroy; bookkeeping)
    bool on = true;
    DevBlockCache()
    {
        const char* e = getenv("ICPMI_ALLOC_CACHE_MB");
        const long mb = e ? atol(e) : 1024;                // r6: 1 GiB (r5: 4 GiB -- a co-resident allocator sees cached blocks as used memory)
        on = mb > 0; limit = on ? (size_t)mb << 20 : 0;
    }
};
inline DevBlockCache& dev_block_cache() { static DevBlockCache* c = new DevBlockCache; return *c; } // (never destroyed: the runtime may be gone first)

// every cached block of every device back to the runtime (icpmi_trim_cache; the out-of-memory path -- and nothing else: a destroyed handle,
// the last one included, leaves its blocks cached, api.hip: icpmi_destroy).
// Caller holds bc.mu.  hipFree synchronises the device it runs on; the blocks are idle, so any device will do.
inline void dev_cache_release_locked(DevBlockCache& bc)
{
    for (auto& dv : bc.idle_of) for (auto& kv : dv.second) (void)hipFree(kv.second);
    bc.idle_of.clear(); bc.idle_bytes = 0;
}
inline void dev_cache_trim()
{
    DevBlockCache& bc = dev_block_cache();
    std::lock_guard<std::mutex> lk(bc.mu);
    dev_cache_release_locked(bc);
}

inline hipError_t dev_malloc(void** p, size_t bytes)
{
    DevBlockCache& bc = dev_block_cache();
    if (!bc.on) return hipMalloc(p, bytes);
    if (bytes == 0) bytes = 1;
    bytes = (bytes + 255) & ~(size_t)255;
    int dev = 0;
    (void)hipGetDevice(&dev); // (a handle is created, used and destroyed with its device current: icpmi_create / CHECK_H set it)
    {
        std::lock_guard<std::mutex> lk(bc.mu);
        auto& idle = bc.idle_of[dev];
        auto it = idle.lower_bound(bytes);
        if (it != idle.end() && it->first <= 2 * bytes + ((size_t)1 << 20)) {
            *p = it->second; bc.live[*p] = {it->first, dev}; bc.idle_bytes -= it->first; idle.erase(it);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { // out of memory: give the cache back and try once more
        std::lock_guard<std::mutex> lk(bc.mu);
        (void)hipGetLastError();
        dev_cache_release_locked(bc);
        e = hipMalloc(p, bytes);
        if (e != hipSuccess) return e;
    }
    std::lock_guard<std::mutex> lk(bc.mu);
    bc.live[*p] = {bytes, dev};
    return hipSuccess;
}

// A destroy returns ~80 blocks: ONE device-wide wait under the exclusive capture gate when this scope opens, and every dev_free of the thread
// inside it skips its own (one wait per block stalled every other thread's registration on this GPU ~80 times in a row).  The
// scope covers blocks of the device that is current when it opens (icpmi_destroy: the handle's).
struct DevFreeSynced {
    static int& depth() { static thread_local int d = 0; return d; }
    DevFreeSynced() { std::unique_lock<std::shared_mutex> gate(capture_gate()); (void)hipDeviceSynchronize(); ++depth(); }
    ~DevFreeSynced() { --depth(); }
    DevFreeSynced(const DevFreeSynced&) = delete;
    DevFreeSynced& operator=(const DevFreeSynced&) = delete;
};

inline hipError_t dev_free(void* p)
{
    if (!p) return hipSuccess;
    DevBlockCache& bc = dev_block_cache();
    if (!bc.on) return hipFree(p);
    DevBlockCache::Live lv{0, 0};
    {
        std::lock_guard<std::mutex> lk(bc.mu);
        auto it = bc.live.find(p);
        if (it == bc.live.end()) return hipFree(p); // not ours (allocated before the cache was switched on)
        lv = it->second; bc.live.erase(it);
    }
    hipError_t e = hipSuccess;
    if (!DevFreeSynced::depth()) {
        // what hipFree would have waited for -- on the device the block lives on; not while another thread captures
        std::unique_lock<std::shared_mutex> gate(capture_gate());
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != lv.dev) (void)hipSetDevice(lv.dev);
        e = hipDeviceSynchronize();
        if (cur != lv.dev) (void)hipSetDevice(cur);
    }
    std::lock_guard<std::mutex> lk(bc.mu);
    bc.idle_of[lv.dev].emplace(lv.bytes, p); bc.idle_bytes += lv.bytes;
    while (bc.idle_bytes > bc.limit) { // the largest block of the fullest device goes first
        std::multimap<size_t, void*>* big = nullptr;
        for (auto& dv : bc.idle_of) if (!dv.second.empty() && (!big || std::prev(dv.second.end())->first > std::prev(big->end())->first)) big = &dv.second;
        if (!big) break;
        auto last = std::prev(big->end());
        (void)hipFree(last->second); bc.idle_bytes -= last->first; big->erase(last);
    }
    return e;
}

// ------------------------------------------------------------------------------------------------
// DevArr<T>: a device array that OWNS its block -- pointer and capacity (in entries) as one unit.  Every device array a handle keeps
// (icpmi_ctx, SelfGridCtx) and every per-call block (DevBuf) is one: it frees itself through dev_free when it dies, a ping-pong exchange
// is one swap(a, b), and it reads as a T* wherever a pointer is expected.  It cannot be copied (`auto p = c->d_x;` does not compile) and
// its address cannot be taken (`(void**)&c->d_x` would write a pointer past its capacity).
// Everything that is a plain pointer BORROWS: GridLevels::pts / cs / pos0, the pointers of an NnRequest, qsorted_src, d_state_mirror,
// d_progress, d_nocc_host, kernel arguments -- views of blocks some DevArr (or pinned host memory) owns, never freed through them.
// The growth rule is part of the type: how much more than asked for a reallocation takes decides which requests the block cache can serve
// and how much HBM a long run holds.
// ------------------------------------------------------------------------------------------------
struct icpmi_ctx;
// doubling: a map that grows by a scan's worth of points per update would otherwise reallocate a few of its ~20 arrays on every
// update, and a hipFree is a device-wide synchronisation (~0.2 ms each, r3 HIP trace: 1 ms per map update); HBM is not the constraint
struct GrowDouble { static size_t want(size_t need) { return 2 * need + 64; } static constexpr bool drains_stream = false; };
// the self grid's tables follow the cloud closely (a quarter of headroom); the handle's stream is drained before a block is given back
struct GrowQuarter { static size_t want(size_t need) { return need + need / 4 + 64; } static constexpr bool drains_stream = true; };
// operator scratch, in bytes
struct GrowScratch { static size_t want(size_t need) { return 2 * need + 256; } static constexpr bool drains_stream = true; };

template <typename T, class Grow = GrowDouble>
class DevArr {
    T* p = nullptr;
    size_t cap = 0;
public:
    DevArr() = default;
    DevArr(const DevArr&) = delete;
    DevArr& operator=(const DevArr&) = delete;
    DevArr(DevArr&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevArr& operator=(DevArr&& o) noexcept { swap(*this, o); return *this; }
    ~DevArr() { (void)reset(); }
    DevArr* operator&() = delete;
    friend void swap(DevArr& a, DevArr& b) noexcept { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
    T* get() const { return p; }
    size_t capacity() const { return cap; }
    hipError_t reset() { const hipError_t e = dev_free(p); p = nullptr; cap = 0; return e; }
    // a block of exactly n entries (an empty array only: what is allocated once, or per call)
    hipError_t alloc(size_t n)
    {
        if (p) return hipErrorInvalidValue;
        if (!n) n = 1;
        const hipError_t e = dev_malloc((void**)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
    // at least `need` entries, contents undefined; *fresh = true when the block is a new one.  Errors: last_error, ICPMI_ERR_HIP.
    icpmi_status ensure(icpmi_ctx* c, size_t need, bool* fresh = nullptr);
    // ... the first `used` entries survive a reallocation
    icpmi_status ensure_keep(icpmi_ctx* c, size_t need, size_t used);
};
// scratch device allocation of one call: freed on every exit path (dev_free waits for work still using it)
template <typename T> using DevBuf = DevArr<T>;

// Streams through a process-wide pool (r5): hipStreamCreateWithFlags takes 1.7 - 23 ms on this runtime and hipStreamDestroy 2 - 3.5 ms
// (rocprofv3 --hip-runtime-trace on the BASELINE config 4 replay: 10 creations = 50 ms of a run whose 42 scans take 130 ms) -- a mapper
// that is built, fed a trajectory and dropped paid for its handle's stream, the private handle of its map-side operators and the side
// stream of its chain with its first two scans.  A released stream is drained and kept (at most 16).
struct StreamPool { std::mutex mu; std::map<int, std::vector<hipStream_t>> idle_of; }; // per device
inline StreamPool& stream_pool() { static StreamPool* p = new StreamPool; return *p; }
inline hipError_t stream_acquire(hipStream_t* s)
{
    StreamPool& sp = stream_pool();
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> lk(sp.mu);
        auto& idle = sp.idle_of[dev];
        if (!idle.empty()) { *s = idle.back(); idle.pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
inline void stream_release(hipStream_t s)
{
    if (!s) return;
    (void)hipStreamSynchronize(s);
    StreamPool& sp = stream_pool();
    int dev = 0;
    (void)hipGetDevice(&dev); // (a handle is created, used and destroyed with its device current: icpmi_create / CHECK_H set it)
    {
        std::lock_guard<std::mutex> lk(sp.mu);
        auto& idle = sp.idle_of[dev];
        if (idle.size() < 16) { idle.push_back(s); return; }
    }
    (void)hipStreamDestroy(s);
}

// One level of a VoxelMatcher handle (voxel.hip): the occupied voxels' keys and records in ascending key order and
// the open-addressing table (64-byte slots, mask + 1 of them) the kernels probe, built for `built_size`.  gen counts the level's builds.
#define ICPMI_MAX_VOXEL_LEVELS 4
struct VoxLevel {
    DevArr<unsigned long long> keys; DevArr<float4> rec; DevArr<uint4> tab;
    int64_t nv = 0; unsigned mask = 0; bool ready = false;
    uint64_t map_version = 0, epoch = 0, gen = 0; float built_size = 0.f;
};
// The occupancy pyramid of the global localisation search (occupancy.hip): per level l the keys of occB_l in ascending order
// and an open-addressing table of key-only 8-byte slots (mask + 1 of them, the smallest power of two >= 2 x keys).  Built lazily for
// (map_version, map_epoch, s0, levels) and kept until one of them changes.  cell_lo / cell_hi: the extent of occ0, the default window.
#define ICPMI_MAX_OCC_LEVELS 8
struct OccLevel { DevArr<unsigned long long> keys, tab; int64_t nk = 0; unsigned mask = 0; float build_ms = 0.f; };
struct OccPyramid {
    OccLevel lv[ICPMI_MAX_OCC_LEVELS];
    int levels = 0; float s0 = 0.f; bool ready = false;
    uint64_t map_version = 0, epoch = 0, builds = 0;
    int cell_lo[3] = {0, 0, 0}, cell_hi[3] = {0, 0, 0};
};
// The device block of a scheduled handle (two or more levels), in dwords: 16 of level descriptors (per level: table address lo, hi, mask,
// size bits -- voxel_pairs_sched_kernel takes them in one load, lane l dword l), then what voxel_advance_kernel keeps between iterations:
// the iteration count at which the current level began, and per level the iterations run and the pair counts of its first and last
// iteration.  The current level itself is the loop header's vox_level.
#define ICPMI_VS_DESC 0
#define ICPMI_VS_BASE 16
#define ICPMI_VS_ITERS 17
#define ICPMI_VS_FIRST 21
#define ICPMI_VS_LAST 25
#define ICPMI_VS_WORDS 32

// The 63-bit key of a cell, shared by the VoxelMatcher tables (voxel.hip) and the occupancy pyramid (occupancy.hip)
constexpr unsigned long long VOX_EMPTY = ~0ull;          // (a key has 63 bits: never all ones)
constexpr float VOX_RANGE = 1048576.f;                   // |index| < 2^20 on every axis
constexpr int VOX_BIAS = 1 << 20;

// The key of a centred point: per axis i = (int)floorf(x / size) in float32 (the division correctly rounded), biased by 2^20 into 21 bits;
// x in the top field, so ascending keys are ascending (ix, iy, iz).  false: a coordinate is not finite or an index is out of range.
__host__ __device__ __forceinline__ bool vox_key(float x, float y, float z, float size, unsigned long long* key)
{
    const float fx = floorf(x / size), fy = floorf(y / size), fz = floorf(z / size);
    if (!(fabsf(fx) < VOX_RANGE && fabsf(fy) < VOX_RANGE && fabsf(fz) < VOX_RANGE)) return false; // (NaN and +-inf fail here too)
    *key = ((unsigned long long)((int)fx + VOX_BIAS) << 42) | ((unsigned long long)((int)fy + VOX_BIAS) << 21) | (unsigned long long)((int)fz + VOX_BIAS);
    return true;
}
// where a key's probe sequence starts (include/icpmi.h states it: tests build colliding key sets from it)
__host__ __device__ __forceinline__ unsigned vox_hash(unsigned long long key, unsigned mask)
{
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

#define ICPMI_SCRATCH_SLOTS 24
struct icpmi_ctx {
    icpmi_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;
    // Every public entry point holds this for its whole duration: the handle's stream, staging buffers, operator scratch and
    // `temp` handle are shared by all calls, and the reference's callers reach one handle from several threads (online mode:
    // input filters on the caller's thread, the map update on a std::async thread, cell paging on Map::updateThread --
    // Mapper.cpp:274-288, Map.cpp:35-57).  Recursive: entry points call each other.
    std::recursive_mutex mu;

    // map
    int64_t m = 0;
    float mean[3] = {0, 0, 0};
    GridParams grid{};
    int64_t n_occupied = 0;
    DevArr<float4> d_map_sorted;        // xyz centred, w = bits of the original index
    DevArr<float4> d_normals_sorted;    // xyz normal, w unused; unused if the map has no normals
    // point and normal of level-0 position s side by side (pn[2 s], pn[2 s + 1]: one 64-byte sector): what the pair sums of a k > 1
    // chain gather at random -- two separate 16-byte gathers fetch two sectors (r3: 76.5 MB per launch for 33.6 MB of payload)
    DevArr<float4> d_map_pn;
    DevArr<unsigned> d_cell_start;      // ncells + 1
    bool has_normals = false;
    // coarser pyramid levels (level 0 aliases d_map_sorted / d_cell_start)
    GridLevels levels{};
    DevArr<uint4> d_lvl_tab;            // device copy of `levels` as 4 x uint4 per level (nn.hip reads it into LDS)
    DevArr<float4> d_lvl_pts[ICPMI_MAXLEV];
    DevArr<unsigned> d_lvl_cs[ICPMI_MAXLEV];
    DevArr<unsigned> d_lvl_pos0[ICPMI_MAXLEV];
    DevArr<unsigned> d_inv;             // original index -> level-0 position (kept for the incremental insert, map_build.hip: map_insert)
    // r4: incremental index insert.  A map that grew by an APPEND (Map::updateLocalPointCloud with PointDistanceMapperModule, the merge epoch
    // of the scan-sharded mapper) keeps its grid; its new index is the old one with the delta merged into the cell-sorted arrays of every
    // level -- one streaming pass per level instead of keys + histogram + scan + atomic scatter over all points.  The result is what a
    // full build on the same grid produces up to the order inside a cell (which nothing downstream sees): centred coordinates are
    // recomputed from the raw points with the NEW centroid, bit for bit what map_build writes.
    DevArr<unsigned> d_lvl_key[ICPMI_MAXLEV];// cell of every sorted position, per level
    DevArr<float4> d_alt_pts[ICPMI_MAXLEV];// ping-pong set the merge writes into
    DevArr<unsigned> d_alt_cs[ICPMI_MAXLEV];
    DevArr<unsigned> d_alt_pos0[ICPMI_MAXLEV];
    DevArr<unsigned> d_alt_key[ICPMI_MAXLEV];
    DevArr<float4> d_raw0;              // level-0 twin: the RAW points (w = original index) in level-0 sorted order (centred handles)
    DevArr<float4> d_alt_raw0;
    DevArr<unsigned> d_ins_dstart0;     // level 0's delta prefix, kept while the upper levels are merged
    DevArr<float4> d_alt_nsorted;
    DevArr<float4> d_alt_pn;
    DevArr<unsigned> d_ins_key;         // delta: cell key and rank inside the cell, per level
    DevArr<unsigned> d_ins_rank;
    bool ins_ready = false;            // the current index carries the key / twin arrays the insert needs
    bool ins_normals_changed = false;  // set by a caller that recomputed the normals of the WHOLE cloud before an append-build (ops.hip)
    double sum_raw[3] = {0, 0, 0};     // sum of the raw coordinates of the indexed cloud (the centroid of the grown cloud without a pass over it)
    float lo_raw[3] = {0, 0, 0}, hi_raw[3] = {0, 0, 0}; // its bounding box
    float cell0 = 0.f;                 // level-0 cell edge as chosen by the last full build (the insert keeps it)
    uint64_t raw_epoch = 0;            // bumped whenever d_raw is rewritten other than by an append (private raw index: ops.hip)
    uint64_t temp_raw_epoch = 0; int64_t temp_raw_m = 0;
    uint64_t raw_view_version = 0;     // map_version the raw-frame VIEW of the registration index was set up for (ops.hip: raw_index)
    int64_t raw_view_count = 0;        // PointDistance searches served by the view (diagnostics)
    int64_t ins_count = 0, full_count = 0; // builds served by the insert / by the full path (diagnostics)

    // scratch for set_map
    DevArr<unsigned> d_keys;
    int oct_depth_hint = 0, oct_tag = 0; long oct_respeculated = 0; // octree.hip: tree depth of the previous call on this handle (the sort runs ahead of the depth's arrival), wrong guesses
    DevArr<unsigned> d_fill; bool fill_clean = false; // the count table of the grid builds: zero between builds while fill_clean (map_build.hip: counts_begin)
    DevArr<unsigned> d_blocksums;
    DevArr<double> d_red;

    // reading-side buffers (capacity in entries)
    DevArr<float4> d_reading;           // centred reading
    DevArr<float4> d_read_normals;
    DevArr<float> d_read_noise; int64_t read_noise_n = 0; // simpleSensorNoise of the NEXT reading (one shot)
    DevArr<float> d_read_scalar; int64_t read_scalar_n = 0; // GenericDescriptor{source: reading} row of the NEXT reading
    int64_t read_int_n = 0; // icpmi_set_reading_intensity: the intensity row of the NEXT reading (one shot), n floats behind the n of the row above
    // KDTreeVarDistMatcher (icpmi_set_reading_max_dist): the SQUARED radii of the NEXT reading, caller's order, and the largest radius of
    // the row (un-squared; +inf when an entry is): the one bound the search prunes with
    DevArr<float> d_read_r2; int64_t read_r2_n = 0; float read_r2_max = 0.f;
    DevArr<float4> d_qsorted;           // centred reading sorted by tile (NN locality)
    DevArr<int> d_qindex;               // sorted position -> original index
    DevArr<unsigned> d_qkeys;
    DevArr<unsigned> d_qtile;
    int64_t qsorted_n = -1; const float4* qsorted_src = nullptr; // which reading d_qsorted was built from
    DevArr<float4> d_stage_in;          // host->device staging
    DevArr<float> d_stage_n3;
    // resident copy of the map as it was handed to set_map (original frame, caller's order): what the
    // device-side map update appends to and rebuilds from
    DevArr<float4> d_raw;
    DevArr<float> d_raw_n3;
    int64_t m_raw = 0; bool raw_has_normals = false;
    // one tracked scalar descriptor of the resident map (`probabilityDynamic` for the shipped chain) and the ping-pong
    // set the map-update chain compacts into (ops.hip: ops_map_update_chain)
    DevArr<float> d_raw_s; bool raw_has_scalar = false;
    // the `densities` row a SURFACE_NORMALS step with keepDensities wrote (ops.hip: invalid at the start of every program, valid from that step
    // on, compacted along with the points, resident afterwards; icpmi_get_map_densities hands it out)
    DevArr<float> d_raw_d; bool raw_has_density = false;
    DevArr<int> d_src;                  // provenance of every point of the map being updated
    DevArr<float4> d_alt_raw;
    DevArr<float> d_alt_n3;
    DevArr<float> d_alt_s;
    DevArr<float> d_alt_d;
    DevArr<int> d_alt_src;
    DevArr<float> d_stage_s;
    // scratch of the map-side operators (hash tables, beam buckets, flags): kept between calls -- a hipMalloc / hipFree
    // pair costs more than most of the kernels that use them
    DevArr<unsigned char, GrowScratch> scratch[ICPMI_SCRATCH_SLOTS];// slots 0..9: operators on the handle's stream; 10..19: the DynamicPoints module (may run on `side`); 20..23: sweep registration (sweep.hip)
    hipStream_t side = nullptr;                              // map-update chain: DynamicPoints next to the decimation that follows it (ops.hip)
    hipEvent_t side_fork = nullptr, side_join = nullptr;
    // the scan of the last icpmi_register_prior, in the map frame by its prior (what Mapper::processInput calls `input`)
    DevArr<float4> d_scan_map; int64_t scan_map_n = 0;
    icpmi_ctx* temp = nullptr;        // private handle of the map-side operators (indexes arbitrary clouds), created on first use
    // PointDistanceMapperModule builds its kd-tree on the map AS IT IS (PointDistanceMapperModule.cpp:32-36), the ICP matcher on the
    // map minus its centroid: squared distances in the two frames differ by rounding, and a keep decision at d2 ~ minDist^2 with
    // them.  The resident map-update paths therefore decide against this second index of the resident map in its own frame, rebuilt
    // when the map changed (map_version) -- not against the registration index.
    icpmi_ctx* temp_raw = nullptr; uint64_t temp_raw_version = 0;
    uint64_t map_version = 0;         // bumped by every map_build of this handle
    bool single_level = false;        // the raw-frame VIEW of a registration index (ops.hip: raw_index): level 0 of the pyramid is all it searches
    bool keep_raw = true;             // temp handles index clouds they do not own: no resident copy of the input
    bool no_centre = false;           // temp handles of the map-side operators: index raw coordinates (mean = 0)
    bool is_raw_index = false;        // the private raw-frame index of a resident map (ops.hip: raw_index): grows by appends with its owner
    DevArr<int> d_sidx;                 // k x n sorted-map index (-1 none)
    DevArr<float> d_d2;                 // k x n
    DevArr<unsigned> d_hard;            // hard query list
    DevArr<unsigned> d_selhist;         // ICPMI_SELHIST_WORDS per reading of a batch
    DevArr<float4> d_match_pt;          // k = 1 loop: matched map point (xyz, original index bits) per query slot
    // k = 1 loop of a single reading: three defer lists of 8 * nn_defer_wgs query slots, then one flag word per query slot (nn.hip:
    // nn1_wg_kernel).  nn_defer / nn_defer_wgs: ICPMI_NN_DEFER (0 = off) and ICPMI_NN_DEFER_WGS as the handle found them when it was created.
    DevArr<unsigned> d_defer;
    bool nn_defer = true; int nn_defer_wgs = ICPMI_NN_DEFER_WGS_DEFAULT;
    // what icpmi_debug_last_matches reads: n and k of the last single registration whose matches are still in d_sidx / d_d2 (0 = none), and
    // whether they are in the tile-sorted query order (d_qindex).  Cleared by everything else that writes those buffers or moves the map.
    int64_t last_match_n = 0; int last_match_k = 0; bool last_match_sorted = false;
    // icpmi_get_covariance (loop.hip: loop_covariance): per-workgroup partials of H / S, then the 36 floats of Cov; cov_ready = computed
    // for the last single registration (read only while last_match_n says its pairs are still the ones in the buffers)
    DevArr<double> d_cov; bool cov_ready = false;
    bool cov_kept = false; // an icpmi_residual_error* call reused the matcher's buffers behind that registration: d_cov still holds its covariance
    // icpmi_debug_keep_sums: 32 doubles the solve kernel of a single registration writes its pair sums to (null: not kept, the default --
    // the same launches with sums_out == nullptr); read by icpmi_debug_last_sums under the condition of icpmi_debug_last_matches
    DevArr<double> d_keep_sums;
    // icpmi_get_localizability: the side block of the degeneracy-aware solve (ICPMI_DG_*; allocated when a chain first asks for it) and
    // whether it holds the report of the last single registration (cleared by batches, multistart and whatever clears cov_ready)
    DevArr<double> d_degen; bool degen_ready = false;
    // icpmi_set_plane_epsilon: epsilon of the plane-to-plane minimiser's covariances; handle state (icpmi_set_config leaves it), carried into
    // the kernels -- and into the signature of a cached loop graph -- by make_loop_cfg
    float plane_eps = 1e-3f;
    // icpmi_set_plane_pair_model: the pair model ICPMI_MIN_PLANE_TO_PLANE runs (ICPMI_PLANE_MODEL_*); handle state like plane_eps, and carried likewise
    int plane_model = ICPMI_PLANE_MODEL_GICP;
    // icpmi_set_intensity_weight: 1 - lambdaGeometric of the photometric term on ICPMI_MIN_POINT_TO_PLANE (0: off); handle state like plane_eps,
    // and carried likewise.  icpmi_set_map_intensity: (g.x, g.y, g.z, I) per map point in the index's order, valid for the index of map_version
    // gi_version with gi_m points -- every map_build moves on and thereby drops the channel
    float intensity_w = 0.f;
    DevArr<float4> d_map_gi; uint64_t gi_version = 0; int64_t gi_m = 0;
    // icpmi_set_voxel_schedule / icpmi_set_voxel_matcher: the voxel sizes, coarsest first (vox_levels = 0: off); handle state like
    // plane_eps.  voxel_size is the finest of them, the size of a one-size handle.  One table of the resident map per level (VoxLevel), built
    // lazily by voxel_ensure_table; a level is current while the map (map_version, map_epoch) and its size are those it was built for.
    // loop_sig hashes the level count and every level's size, generation and table address: none is part of the LoopCfg.
    // d_vox_sched (ICPMI_VS_WORDS dwords; two or more levels): the level descriptors as uploaded for vox_sched_sig, and the advance's report.
    // vox_step_level: the level icpmi_minimize_step_normals evaluates (-1: the finest; icpmi_debug_voxel_step_level).  vox_report: the last
    // registration's levels entered, then per level iterations, first and last pair count (icpmi_get_voxel_schedule_report).
    float voxel_size = 0.f;
    int vox_levels = 0; float vox_sizes[ICPMI_MAX_VOXEL_LEVELS] = {0.f, 0.f, 0.f, 0.f};
    VoxLevel vox[ICPMI_MAX_VOXEL_LEVELS];
    DevArr<unsigned> d_vox_sched; uint64_t vox_sched_sig = 0;
    int vox_step_level = -1;
    int32_t vox_report[1 + 3 * ICPMI_MAX_VOXEL_LEVELS] = {0};
    // a batch on the voxel path: d_vox_batch = ICPMI_VS_WORDS dwords with the level descriptors every member reads (one
    // level for a one-size handle), then ICPMI_VS_WORDS per member for its own report (voxel.hip: voxel_ensure_batch_block).
    // vox_batch_report: per member of the last batch or multistart what vox_report is for a registration; vox_batch_members: how many
    DevArr<unsigned> d_vox_batch; uint64_t vox_batch_sig = 0;
    int32_t vox_batch_report[ICPMI_MAX_BATCH][1 + 3 * ICPMI_MAX_VOXEL_LEVELS] = {{0}};
    int vox_batch_members = 0;
    OccPyramid occ;                   // icpmi_global_localize* and the occupancy calls (occupancy.hip); nothing else reads it
    // test seam (icpmi_debug_voxel_batch_calls): loops of loop_run_voxel_batch, members they carried, single registrations on the voxel path
    int64_t vox_batch_loops = 0, vox_batch_loop_members = 0, vox_single_regs = 0;
    DevArr<IcpState> d_state;         // ICPMI_MAX_BATCH states (a single registration uses the first)
    IcpState* h_state = nullptr;                               // pinned mirror (ICPMI_MAX_BATCH)
    bool zero_pending = false;                                 // d_state / d_selhist still to be cleared: on the stream the handle really uses, at its first call (zero_state_if_pending)
    unsigned scan_tag = 0;                                     // call number of device_scan_flags_count: the tag its count comes back with (map_build.hip)
    IcpState* d_state_mirror = nullptr;                        // ... and its device address: the solve kernel of a single registration writes the finished state there itself (r5)
    unsigned* d_nocc_host = nullptr; bool nocc_by_scan = false; // device address of h_nocc; the pending occupancy word is delivered by the build's scan
    unsigned* h_nocc = nullptr; int64_t nocc_m = 0;            // pinned word: occupied cells of the last index build, and that build's point count (map_build)
    unsigned char* h_pin = nullptr;                            // pinned page: [0, ICPMI_PIN_BYTES) small read-backs, behind it the ring of upload_small
    unsigned up_next = 0;
    // Progress word of the running registration in host-mapped pinned memory, written by the solve kernel after every
    // iteration: bit 31 = loop finished, bits 30..12 = registration sequence number, bits 11..0 = iterations completed.
    // A registration with data-dependent length (Differential / Bound checkers) is enqueued eagerly, a bounded number of
    // iterations ahead of this word, instead of stopping the stream for a read-back every few iterations (loop.hip).
    unsigned* h_progress = nullptr; unsigned* d_progress = nullptr; unsigned reg_seq = 0;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> nn_events;

    LoopGraphs graphs;                // the cached loop graphs (checked loops: Counter + Differential / Bound, what Mapper::processInput runs)
    int seg_wasted = 0, graph_wasted = 0; uint64_t eager_sig = 0, map_epoch = 0;   // see drop_loop_graphs (map_epoch: one tick per invalidation)
    int seg_prev_iters = 0, seg_last_iters = 0;

    // buffers of the map-growth epoch (ops.hip: ops_staged_merge_allgather): this rank's accepted points, all ranks' blocks, the merged set
    DevArr<float4> d_merge_send;
    DevArr<float4> d_merge_recv;
    DevArr<float4> d_merged;
    // RCCL communicator of the scan-sharded mapping mode (comm.hip); null = a single rank
    void* comm = nullptr; int comm_ranks = 1, comm_rank = 0;
    float comm_loop_shift = 0.f;      // loopback communicator (comm.hip): rank r's block = this rank's, moved r * shift along x
    bool comm_loop_ragged = false;    // ... and cut to unequal sizes (comm.hip: loop_counts_kernel)
    DevArr<long long> d_comm_cnt;       // words of the epoch's count / ready exchanges (allocated by comm_init)
    // r5: the ONE-collective epoch (ops.hip: ops_staged_merge_allgather).  Every rank hands in a block of merge_block + 1 float4: a header
    // {bits(count) | -1, magic} and up to merge_block accepted points; the blocks are sized when the communicator is created (no allocation,
    // hence no `ready` exchange, between the local accept and the collective).  0: the three-collective epoch of r4.
    int64_t merge_block = 0;
    long merge_fast_epochs = 0, merge_slow_epochs = 0; // epochs served by the one-collective path / by the count + ready + points path
    int64_t merged_last_n = 0;        // points of the last epoch's merged set, still in d_merged (icpmi_staged_merged_points)
    // r6 (cells.hip): every merged set binned by icpmi_staged_bin_cells, cell after cell; the host keeps {offset, count} runs per cell id
    DevArr<float4> d_cell_log; int64_t cell_log_n = 0;
    // r6 (ops.hip: surface_normals_dev): d^2 of the k-th neighbour of every resident point as the last SurfaceNormal pass over the resident map found it
    // (original order) -- an append recomputes only the normals an appended point can have changed.  Valid for the first dk_m points while
    // dk_epoch == raw_epoch (nobody rewrote the resident copy) and the filter's knn is dk_knn.
    DevArr<float> d_raw_dk; int64_t dk_m = 0; int dk_knn = 0; uint64_t dk_epoch = ~0ull;
    long normals_incremental = 0, normals_full = 0; int64_t normals_last_searched = 0;   // diagnostics (icpmi_debug_counters 20 / 21 / 22)
    DevArr<unsigned> d_patch_unplaced; // one word: changed normals whose sorted copy patch_normals_kernel did not find, since the handle was created (icpmi_debug_counters 23)
    bool merged_binned = false;       // the merged set of the last epoch is in the log already
    int cell_bits_hint = 0;           // key bits the previous epoch's cell count needed (the sort is enqueued before the count is known)
    float cell_auto_size = 0.f;       // > 0 (icpmi_cell_log_configure): every epoch enqueues the binning of its merged set itself, behind the merge
    unsigned char* h_cells = nullptr; // pinned: header + cell table of the binning in flight
    int64_t cells_enq_n = 0; int cells_enq_bits = 0; float cells_enq_size = 0.f;   // what is enqueued and not yet collected (n == 0: nothing)
    struct SelfGridCtx* sg = nullptr; // sparse block grid of the self k-NN (selfgrid.hip): tables, work lists and the tuning state of the handle's previous build
    bool counted = false;             // created through icpmi_create (not a private handle): counts towards the allocation cache's lifetime (api.hip)
};

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);             \
            return ICPMI_ERR_HIP;                                                              \
        }                                                                                      \
    } while (0)

template <typename T, class Grow>
icpmi_status DevArr<T, Grow>::ensure(icpmi_ctx* c, size_t need, bool* fresh)
{
    if (need <= cap && p) return ICPMI_OK;
    if (p) {
        if (Grow::drains_stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, reset());
    }
    const size_t want = Grow::want(need);
    HIP_TRY(c, dev_malloc((void**)&p, want * sizeof(T)));
    cap = want;
    if (fresh) *fresh = true;
    return ICPMI_OK;
}
template <typename T, class Grow>
icpmi_status DevArr<T, Grow>::ensure_keep(icpmi_ctx* c, size_t need, size_t used)
{
    if (need <= cap && p) return ICPMI_OK;
    const size_t want = Grow::want(need);
    T* q = nullptr;
    HIP_TRY(c, dev_malloc((void**)&q, want * sizeof(T)));
    if (p && used) HIP_TRY(c, hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    if (p) { HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, reset()); }
    p = q; cap = want;
    return ICPMI_OK;
}

// Every cached loop graph (fixed-count, batched, the segment and head graphs of a checked loop) holds pointers, grid parameters, the map's
// mean and its normals flag as they were at capture time: a rebuilt index or a changed stream invalidates all of them (only the
// fixed-count graph was dropped, and the signatures do not cover mean / m / has_normals / d_map_pn / the level arrays).
// The loop state and the selection histograms of a new handle are cleared at its FIRST call, on the stream it then has: a private handle adopts its
// owner's stream right after its creation and never touches its own -- clearing there at creation (r5, after the synchronous hipMemset on the
// legacy stream had to go: it breaks another thread's capture) made the runtime build a hardware queue for every such stream, milliseconds
// of the first scans of a mapper.
static inline icpmi_status zero_state_if_pending(icpmi_ctx* c)
{
    if (!c->zero_pending) return ICPMI_OK;
    HIP_TRY(c, hipMemsetAsync(c->d_state, 0, sizeof(IcpState) * ICPMI_MAX_BATCH, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_selhist, 0, ICPMI_SELHIST_WORDS * sizeof(unsigned), c->stream));
    c->zero_pending = false;
    return ICPMI_OK;
}

// icpmi_set_map_intensity's channel belongs to the index it was computed for
static inline bool map_intensity_ready(const icpmi_ctx* c) { return c->d_map_gi.get() && c->gi_m > 0 && c->gi_m == c->m && c->gi_version == c->map_version; }

static inline void drop_loop_graphs(icpmi_ctx* c)
{
    // (r5) graphs that served a single registration before the map under them changed were not worth their capture: two such sets in a
    // row and loop_run goes eager until a signature repeats (a mapper rebuilds its map behind every scan)
    if (c->graphs.fixed.exec) c->graph_wasted = c->graphs.fixed.uses <= 1 ? c->graph_wasted + 1 : 0;
    if (c->graphs.seg[0].exec) c->seg_wasted = c->graphs.seg[0].uses <= 1 ? c->seg_wasted + 1 : 0;
    ++c->map_epoch;
    c->graphs.reset();
    c->last_match_n = 0; c->cov_kept = false;
    c->degen_ready = false; // (the report's pivot is kept in the centred frame of the map it was registered against: gone with that map)
}

// Small device -> host read through the pinned page: a copy into pageable memory is staged and blocks for tens of
// microseconds, and a map update makes a dozen of them (counts after every compaction, grid statistics).
#define ICPMI_PIN_BYTES (128 * 1024)
#define ICPMI_PROGRESS_WORDS 512      // size of the host-mapped page in words
#define ICPMI_PROGRESS_HDR_WORD 64    // ... 256 words: the block headers (counts) of a one-collective epoch, one per rank (ops.hip)
#define ICPMI_MERGE_MAGIC 0x49435035u // 'ICP5' in the header's y
#define ICPMI_PROGRESS_OCT_WORD 48  // ... and 8 words for the octree's root cube (octree.hip)
#define ICPMI_PROGRESS_SELF_WORD 56 // ... two words: sum over the A-cells of (points in the cell)^2 of the handle's last self search (selfgrid.hip: the next build tunes its edge with it)
#define ICPMI_PROGRESS_VOX_WORD 320  // ... 13 words: the report of a scheduled VoxelMatcher registration (voxel.hip: voxel_advance_kernel), final behind the "done" word
#define ICPMI_PROGRESS_SCAN_WORD 40 // word of the host-mapped progress page (api.hip: h_progress, 64 words) that device_scan_flags_count reports into

// Host wait on `count` words of host-mapped memory that the stream's kernels write: spins on them (v = a fresh snapshot) until ready(v),
// and asks the stream every `cadence` spins (a power of two) whether anything is still to run.  A stream in an error state ends the wait
// with its error (nothing will ever write the words); an idle stream means the words are final: v is read once more and *idle set.
template <class T, class Ready>
static inline hipError_t spin_on_host(hipStream_t stream, unsigned cadence, const T* src, int count, T* v, Ready ready, bool* idle = nullptr)
{
    auto load = [&] { for (int i = 0; i < count; ++i) v[i] = __atomic_load_n(src + i, __ATOMIC_ACQUIRE); };
    if (idle) *idle = false;
    for (unsigned spins = 1;; ++spins) {
        load();
        if (ready((const T*)v)) return hipSuccess;
        if ((spins & (cadence - 1)) != 0) continue;
        const hipError_t qe = hipStreamQuery(stream);
        if (qe == hipErrorNotReady) continue;
        if (qe == hipSuccess) { load(); if (idle) *idle = true; }
        return qe;
    }
}
static inline icpmi_status read_back2(icpmi_ctx* c, void* dst0, const void* src0, size_t b0, void* dst1, const void* src1, size_t b1)
{
    if (!c->h_pin || b0 + b1 > ICPMI_PIN_BYTES) {
        HIP_TRY(c, hipMemcpyAsync(dst0, src0, b0, hipMemcpyDeviceToHost, c->stream));
        if (b1) HIP_TRY(c, hipMemcpyAsync(dst1, src1, b1, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return ICPMI_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_pin, src0, b0, hipMemcpyDeviceToHost, c->stream));
    if (b1) HIP_TRY(c, hipMemcpyAsync(c->h_pin + b0, src1, b1, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    memcpy(dst0, c->h_pin, b0);
    if (b1) memcpy(dst1, c->h_pin + b0, b1);
    return ICPMI_OK;
}
static inline icpmi_status read_back(icpmi_ctx* c, void* dst, const void* src, size_t bytes) { return read_back2(c, dst, src, bytes, nullptr, nullptr, 0); }

// Small host -> device upload (a 4x4, a level table, a counter) through a ring of slots in the pinned page: a copy from PAGEABLE memory is
// staged by the runtime and costs ~40 us of host time each (r3 HIP trace: ~20 of them per map update); from pinned memory it is an async
// DMA of a few microseconds.  The ring lives in the upper half of the page (read-backs use the lower half); 64 slots of 1 KiB: a slot is
// reused only 64 uploads later, and every entry point synchronises its stream long before that.
#define ICPMI_UP_SLOT 1024
#define ICPMI_UP_SLOTS 64
static inline icpmi_status upload_small(icpmi_ctx* c, void* d_dst, const void* h_src, size_t bytes)
{
    if (!c->h_pin || bytes > ICPMI_UP_SLOT) {
        HIP_TRY(c, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
        return ICPMI_OK;
    }
    unsigned char* slot = c->h_pin + ICPMI_PIN_BYTES + (size_t)(c->up_next++ % ICPMI_UP_SLOTS) * ICPMI_UP_SLOT;
    memcpy(slot, h_src, bytes);
    HIP_TRY(c, hipMemcpyAsync(d_dst, slot, bytes, hipMemcpyHostToDevice, c->stream));
    return ICPMI_OK;
}

// slot `k` of the operator scratch, at least `count` entries of T (contents undefined)
template <typename T>
static inline T* scratch_get(icpmi_ctx* c, int k, size_t count)
{
    if (c->scratch[k].ensure(c, (count ? count : 1) * sizeof(T)) != ICPMI_OK) { c->last_error = "out of device memory (operator scratch)"; return nullptr; }
    return (T*)c->scratch[k].get();
}

// ---- device helpers -------------------------------------------------------------------------
__device__ __forceinline__ float3 xf_point(const float* __restrict__ T, float x, float y, float z, float w)
{
    // Same evaluation order as the oracle: column-by-column accumulation with fused multiply-adds.
    float3 o;
    o.x = fmaf(T[12], w, fmaf(T[8], z, fmaf(T[4], y, T[0] * x)));
    o.y = fmaf(T[13], w, fmaf(T[9], z, fmaf(T[5], y, T[1] * x)));
    o.z = fmaf(T[14], w, fmaf(T[10], z, fmaf(T[6], y, T[2] * x)));
    return o;
}

__device__ __forceinline__ float sqdist3(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

__device__ __forceinline__ unsigned long long pack_key(float d2, unsigned id)
{
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)id;
}

// a square root that never under-estimates (one v_sqrt_f32, 1 ulp, nudged up)
__device__ __forceinline__ float sqrt_up(float x) { return __builtin_amdgcn_sqrtf(x) * 1.0000005f; }

// ---- the pieces every grid matcher of nn.hip is written on ("Shared pieces of the matcher kernels") ----
typedef float vf4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vf4 gfloat4;          // 16 bytes in global memory (global_load, not flat_load)
typedef __attribute__((address_space(1))) unsigned gunsigned;

// Readers of the level table (LevelRow) over the uint4 view a kernel keeps of it, in LDS or in global memory.  A pointer rebuilt from
// integers would be read through the flat path: P names the address space, global by default.
__device__ __forceinline__ GridParams level_grid(const uint4* ltab, int lv)
{
    const uint4 a = ltab[4 * lv], b = ltab[4 * lv + 1], c = ltab[4 * lv + 2];
    GridParams g;
    g.ox = __uint_as_float(a.x); g.oy = __uint_as_float(a.y); g.oz = __uint_as_float(a.z); g.cell = __uint_as_float(a.w);
    g.inv_cell = __uint_as_float(b.x); g.slack = __uint_as_float(b.y); g.nx = (int)b.z; g.ny = (int)b.w;
    g.nz = (int)c.x; g.ncells = (int)c.y;
    return g;
}
template <class P = const gfloat4*>
__device__ __forceinline__ P level_pts(const uint4* ltab, int lv) { const uint4 c = ltab[4 * lv + 2]; return reinterpret_cast<P>(((unsigned long long)c.w << 32) | c.z); }
template <class P = const gunsigned*>
__device__ __forceinline__ P level_cs(const uint4* ltab, int lv) { const uint4 d = ltab[4 * lv + 3]; return reinterpret_cast<P>(((unsigned long long)d.y << 32) | d.x); }
template <class P = const gunsigned*>
__device__ __forceinline__ P level_pos0(const uint4* ltab, int lv) { const uint4 d = ltab[4 * lv + 3]; return reinterpret_cast<P>(((unsigned long long)d.w << 32) | d.z); }

// where a point sits in a level: scaled coordinates, their floors, the integer cell (clamped: far outside the box stays representable) and
// mf = the distance to the nearest face of its own cell, in cells (0 for a NaN coordinate: no margin is ever claimed for it)
struct CellPos {
    float fx, fy, fz, flx, fly, flz;
    int cx, cy, cz;
    float mf;
};
__device__ __forceinline__ CellPos cell_pos(float x, float y, float z, const GridParams& g)
{
    CellPos c;
    c.fx = (x - g.ox) * g.inv_cell; c.fy = (y - g.oy) * g.inv_cell; c.fz = (z - g.oz) * g.inv_cell;
    c.flx = floorf(c.fx); c.fly = floorf(c.fy); c.flz = floorf(c.fz);
    c.cx = (int)fminf(fmaxf(c.flx, -1.0e6f), 1.0e6f);
    c.cy = (int)fminf(fmaxf(c.fly, -1.0e6f), 1.0e6f);
    c.cz = (int)fminf(fmaxf(c.flz, -1.0e6f), 1.0e6f);
    float mf = fminf(c.fx - c.flx, 1.0f - (c.fx - c.flx));
    mf = fminf(mf, fminf(c.fy - c.fly, 1.0f - (c.fy - c.fly)));
    mf = fminf(mf, fminf(c.fz - c.flz, 1.0f - (c.fz - c.flz)));
    if (!(mf >= 0.f)) mf = 0.f;
    c.mf = mf;
    return c;
}

// The exactness rule of the search.  Every point within block_margin of the query lies inside the (2 ring + 1)^3 block of cells around the
// query's cell: a k-th distance within it decides the query.  block_margin_seed is the same reach claimed BEFORE a search, from a bound
// that was computed elsewhere (two slacks); block_covers: the block holds the whole grid, nothing is left to look at.
__device__ __forceinline__ float block_margin(float mf, float cell, float slack, int ring = 1) { return fmaxf(((float)ring + mf) * cell - slack, 0.f); }
__device__ __forceinline__ float block_margin_seed(float mf, float cell, float slack) { return (1.0f + mf) * cell - 2.0f * slack; }
__device__ __forceinline__ bool block_covers(const CellPos& c, const GridParams& g, int ring = 1)
{
    return c.cx - ring <= 0 && c.cx + ring >= g.nx - 1 && c.cy - ring <= 0 && c.cy + ring >= g.ny - 1 && c.cz - ring <= 0 && c.cz + ring >= g.nz - 1;
}
// the 3 x 3 x 3 block of level g around the point holds the ball of radius ub around it
__device__ __forceinline__ bool block_holds_ball(float x, float y, float z, const GridParams& g, float ub)
{
    return ub <= block_margin_seed(cell_pos(x, y, z, g).mf, g.cell, g.slack);
}
// first level >= from (the top level at the latest) whose block holds that ball
__device__ __forceinline__ int level_holding_ball(const uint4* ltab, int nlev, int from, float x, float y, float z, float ub)
{
    int l = from;
    for (; l < nlev - 1; ++l)
        if (block_holds_ball(x, y, z, level_grid(ltab, l), ub)) break;
    return l;
}

// x-range [xa, xb] of row (dy, dz) of the 3 x 3 x 3 block around c that the ball of squared radius rub2 (+inf: none) around the point can
// reach: the block's own three cells, clipped by what the row's distance leaves of the radius.  false: the ball misses the row.
__device__ __forceinline__ bool clip_row_x(const CellPos& c, const GridParams& g, float x, int dy, int dz, float rub2, int& xa, int& xb)
{
    const float ylo = (c.fy - c.fly) * g.cell, yhi = (1.0f - (c.fy - c.fly)) * g.cell;
    const float zlo = (c.fz - c.flz) * g.cell, zhi = (1.0f - (c.fz - c.flz)) * g.cell;
    const float ddy = dy == 0 ? 0.f : (dy < 0 ? ylo : yhi);
    const float ddz = dz == 0 ? 0.f : (dz < 0 ? zlo : zhi);
    const float rem2 = rub2 - (ddy * ddy + ddz * ddz); // +inf without a bound
    xa = c.cx - 1; xb = c.cx + 1;
    if (rem2 != INFINITY) {
        const float rem = sqrt_up(fmaxf(rem2, 0.f));
        const int xl = (int)fmaxf(floorf((x - rem - g.ox) * g.inv_cell), -1.0e6f);
        const int xh = (int)fminf(floorf((x + rem - g.ox) * g.inv_cell), 1.0e6f);
        xa = xl > xa ? xl : xa;
        xb = xh < xb ? xh : xb;
    }
    return rem2 >= 0.f;
}

// XCD-aware order of a launch's nblocks (a multiple of 8) workgroups: workgroup b runs on XCD b % 8; each XCD gets one contiguous eighth
template <class N>
__device__ __forceinline__ int xcd_block(unsigned b, N nblocks) { const int chunk = nblocks >> 3; return (int)((b & 7) * chunk + (b >> 3)); }

// MurmurHash3's 32-bit finaliser: a bijection of the 32-bit integers, so "smallest hash" names exactly one point
__device__ __forceinline__ unsigned fmix32(unsigned h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}

__device__ __forceinline__ unsigned minstd_mulmod(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) % 2147483647ull); }

// the n-th value (n >= 1) of std::minstd_rand seeded with `seed`: x0 48271^n mod (2^31 - 1) by square-and-multiply -- no sequential generator.
// [rand.predef]: the 10 000th value of a default-constructed (seed 1) minstd_rand is 399268537 (tests/test_gpu_pins.py holds this function to it).
__device__ __forceinline__ unsigned minstd_nth(unsigned seed, unsigned n)
{
    unsigned x = seed % 2147483647u;
    if (x == 0u) x = 1u;
    unsigned e = n, base = 48271u, acc = 1u;
    while (e) { if (e & 1u) acc = minstd_mulmod(acc, base); base = minstd_mulmod(base, base); e >>= 1; }
    return minstd_mulmod(acc, x);
}

// float -> unsigned whose integer order is the float order (-0 sorts below +0), and back
__device__ __forceinline__ unsigned float_key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float float_key_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// false for NaN, +-inf and anything beyond `limit` (FLT_MAX: plain finiteness)
__device__ __forceinline__ bool finite_within(float v, float limit) { return fabsf(v) <= limit; }

// ---- bounding box of a float4 cloud in two stages (octree.hip, voxelgrid.hip, ssn.hip, selfgrid.hip) ----
// Stage 1, bbox_partials_kernel: a grid-stride pass, six floats per workgroup (part[6 b + 0..2] = lo, + 3..5 = hi) and -- COUNT_BAD -- the
// workgroup's number of points with a coordinate that is not finite_within(limit) in bad[b].  Stage 2, bbox_fold: ONE workgroup folds the
// partials (a kernel of the caller's, which goes on to compute what it needs from the box), or the host does after a read-back.  min / max
// are exact, so the box does not depend on the number of workgroups.  (Internal linkage: every file that launches it carries its own copy.)
namespace {
constexpr int BBOX_WG = 256;

// the halving LDS tree over the workgroup's 256 boxes (and counts): every lane leaves with the workgroup's
template <bool COUNT_BAD>
__device__ __forceinline__ void bbox_wg_reduce(float (&lo)[3], float (&hi)[3], unsigned& nbad)
{
    __shared__ float sl[3][BBOX_WG], sh[3][BBOX_WG];
    __shared__ unsigned sb[COUNT_BAD ? BBOX_WG : 1];
    const int t = threadIdx.x;
    for (int r = 0; r < 3; ++r) { sl[r][t] = lo[r]; sh[r][t] = hi[r]; }
    if constexpr (COUNT_BAD) sb[t] = nbad;
    __syncthreads();
    for (int s = BBOX_WG / 2; s > 0; s >>= 1) {
        if (t < s) {
            for (int r = 0; r < 3; ++r) { sl[r][t] = fminf(sl[r][t], sl[r][t + s]); sh[r][t] = fmaxf(sh[r][t], sh[r][t + s]); }
            if constexpr (COUNT_BAD) sb[t] += sb[t + s];
        }
        __syncthreads();
    }
    for (int r = 0; r < 3; ++r) { lo[r] = sl[r][0]; hi[r] = sh[r][0]; }
    if constexpr (COUNT_BAD) nbad = sb[0];
}

template <bool COUNT_BAD>
__global__ __launch_bounds__(BBOX_WG) void bbox_partials_kernel(const float4* __restrict__ pts, int64_t n, float* __restrict__ part,
                                                                unsigned* __restrict__ bad /* COUNT_BAD only */, float limit)
{
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned nb = 0;
    for (int64_t i = (int64_t)blockIdx.x * BBOX_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * BBOX_WG) {
        const float4 p = pts[i];
        if constexpr (COUNT_BAD) nb += (finite_within(p.x, limit) && finite_within(p.y, limit) && finite_within(p.z, limit)) ? 0u : 1u;
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
    bbox_wg_reduce<COUNT_BAD>(lo, hi, nb);
    if (threadIdx.x == 0) {
        for (int r = 0; r < 3; ++r) { part[6 * blockIdx.x + r] = lo[r]; part[6 * blockIdx.x + 3 + r] = hi[r]; }
        if constexpr (COUNT_BAD) bad[blockIdx.x] = nb;
    }
}

// stage 2 inside a kernel of BBOX_WG lanes: the box (and the bad count) of `nparts` partials, in every lane
template <bool COUNT_BAD>
__device__ __forceinline__ void bbox_fold(const float* __restrict__ part, const unsigned* __restrict__ bad, int nparts, float (&lo)[3], float (&hi)[3],
                                          unsigned& nbad)
{
    for (int r = 0; r < 3; ++r) { lo[r] = INFINITY; hi[r] = -INFINITY; }
    nbad = 0;
    for (int b = threadIdx.x; b < nparts; b += BBOX_WG) {
        for (int r = 0; r < 3; ++r) { lo[r] = fminf(lo[r], part[6 * b + r]); hi[r] = fmaxf(hi[r], part[6 * b + 3 + r]); }
        if constexpr (COUNT_BAD) nbad += bad[b];
    }
    bbox_wg_reduce<COUNT_BAD>(lo, hi, nbad);
}
} // namespace

// bounded sorted list of (key = d2 bits << 32 | original index, sorted position): the k best of a k-NN search, in registers
template <int KMAX>
struct KList {
    unsigned long long key[KMAX];
    int sidx[KMAX];
    int k, filled;
    __device__ __forceinline__ void init(int kk)
    {
        k = kk; filled = 0;
#pragma unroll
        for (int i = 0; i < KMAX; ++i) { key[i] = ~0ull; sidx[i] = -1; }
    }
    __device__ __forceinline__ unsigned long long worst() const { return key[KMAX - 1]; }
    // keeps the KMAX smallest; callers read the first k (k <= KMAX), so the list may hold more than
    // k entries -- harmless, and it keeps all indexing static (registers, no scratch).
    __device__ __forceinline__ void insert(unsigned long long kk, int s)
    {
        if (kk >= key[KMAX - 1]) return;
#pragma unroll
        for (int i = KMAX - 1; i >= 0; --i) {
            const unsigned long long prev = i > 0 ? key[i - 1] : 0ull;
            const int prevs = i > 0 ? sidx[i - 1] : -1;
            if (i > 0 && kk < prev) { key[i] = prev; sidx[i] = prevs; }
            else if (kk < key[i]) { key[i] = kk; sidx[i] = s; }
        }
        if (filled < KMAX) ++filled;
    }
};

__device__ inline void quat_from_T(const float* T, double* q)
{
    const double m00 = T[0], m11 = T[5], m22 = T[10];
    double t = m00 + m11 + m22;
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t; t = 0.5 / t;
        q[1] = ((double)T[4 * 1 + 2] - (double)T[4 * 2 + 1]) * t;
        q[2] = ((double)T[4 * 2 + 0] - (double)T[4 * 0 + 2]) * t;
        q[3] = ((double)T[4 * 0 + 1] - (double)T[4 * 1 + 0]) * t;
    } else {
        int i = 0;
        if (m11 > m00) i = 1;
        if (m22 > (i == 0 ? m00 : m11)) i = 2;
        const int j = (i + 1) % 3, kk = (j + 1) % 3;
        auto M = [&](int r, int c) { return (double)T[4 * c + r]; };
        t = sqrt(M(i, i) - M(j, j) - M(kk, kk) + 1.0);
        __shared__ double v[3]; // (run-time index: LDS instead of scratch memory; one lane per workgroup ever gets here)
        v[i] = 0.5 * t; t = 0.5 / t;
        q[0] = (M(kk, j) - M(j, kk)) * t;
        v[j] = (M(j, i) + M(i, j)) * t;
        v[kk] = (M(kk, i) + M(i, kk)) * t;
        q[1] = v[0]; q[2] = v[1]; q[3] = v[2];
    }
}


// start of a registration: the loop state of one reading (init_state_kernel; the last kernel of the query sort when the head is fused)
__device__ inline void init_state_dev(IcpState* st, const float* T0, unsigned seq, unsigned* progress, const unsigned* seq_src)
{
    // seq_src: the sequence number is read from host-mapped memory at RUN time -- a captured graph must not freeze the number of the
    // registration it was captured for (the host matches the progress word against the number of the registration it is waiting on)
    if (seq_src) seq = __hip_atomic_load(seq_src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    st->seq = seq;
    if (progress) __hip_atomic_store(progress, (seq & 0x7ffffu) << 12, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int i = 0; i < 16; ++i) st->T_iter[i] = T0 ? T0[i] : ((i % 5 == 0) ? 1.f : 0.f);
    st->iter = 0; st->done = 0; st->error = 0; st->stop_reason = 0; st->counter = 0;
    quat_from_T(st->T_iter, st->hq);
    for (int r = 0; r < 3; ++r) st->ht[r] = st->T_iter[12 + r];
    for (int r = 0; r < 4; ++r) st->init_q[r] = st->hq[r];
    st->hist_n = 1;
    st->sel_prefix = 0; st->sel_rank = 0; st->n_valid = 0;
    for (int f = 0; f < ICPMI_MAX_OUTLIER; ++f) st->limits[f] = -1.f;
    st->robust_med = 0.f; st->robust_scale = 1.f; st->vt_valid = 0; st->vt_ratio = -1.f;
    st->pairs = 0; st->wsum = 0; st->hard_count = 0; st->hard_total = 0; st->ticket = 0;
    for (int i = 0; i < 24; ++i) st->dbg[i] = 0;
    st->t_nn_begin = 0; st->t_nn_sum = 0; st->nn_count = 0;
    for (int i = 0; i < 3; ++i) st->defer_count[i] = 0;
    st->defer_served = 0; st->defer_overflow = 0;
    st->t_done = 0; // (t_start belongs to the first kernel of the head, which runs BEFORE this when the head is folded into the query sort)
}

// The head of a registration folded into the kernels of the query sort (r3: 8 graph nodes -> 3): the first kernel centres the raw
// readings (Mapper.cpp:213's T_refMean_dataIn) while it computes their tile keys, the last one initialises the loop state and clears
// the selection histograms while it scatters.
struct SortHead {
    BatchSrc raw;                 // the readings as handed in; centred into the sort's input array
    float mean[3];
    IcpState* st = nullptr;       // loop state(s) to initialise (one per reading), or nullptr
    unsigned seq = 0;
    unsigned* progress = nullptr;
    const unsigned* seq_src = nullptr;
    unsigned* selhist = nullptr;  // ICPMI_SELHIST_WORDS words per reading to clear, or nullptr
};

// ---- cross-TU host entry points ---------------------------------------------------------------
// keep_prefix: the first keep_prefix points of d_pts are the cloud of the previous build, unchanged and in the same order (an append)
icpmi_status map_build(icpmi_ctx* c, const float4* d_pts, int64_t m, const float* d_normals3, int64_t keep_prefix = 0);
icpmi_status map_patch_normals(icpmi_ctx* c, const unsigned* d_list, int64_t n_list, const float4* d_raw, const float* d_normals3);
icpmi_status map_patch_unplaced(icpmi_ctx* c, uint64_t* out); // the word behind icpmi_debug_counters 23 (0 while no patch has run)
icpmi_status map_debug_index_normals(icpmi_ctx* c, int64_t m, float* sorted3, float* pn3, int32_t* has_pn); // icpmi_debug_index_normals
icpmi_status upload_level_table(icpmi_ctx* c); // c->levels -> c->d_lvl_tab (the table the NN kernels copy to LDS)
icpmi_status device_exclusive_scan(icpmi_ctx* c, unsigned* data, int n, unsigned total);
icpmi_status device_exclusive_scan_io(icpmi_ctx* c, const unsigned* in, unsigned* out, int n, unsigned total); // in == out allowed
// counts[0..n) -> starts in CURSOR layout (starts[0] = 0, starts[i + 1] = start of cell i, starts[n + 1] = total; n + 2 words): a scatter takes
// its slots with atomicAdd(&starts[key + 1], len) and leaves the plain exclusive scan behind.  zero_counts: counts[0 .. n + 1] end up zero.
icpmi_status device_scan_flags_count(icpmi_ctx* c, const unsigned* flag, unsigned* pos, int n, int64_t* count); // pos = exclusive scan of the 0 / 1 flags, *count = how many are set (one stream wait, no copy)
icpmi_status device_exclusive_scan_sum(icpmi_ctx* c, const unsigned* flag, unsigned* pos, int n, unsigned* d_sum); // ... the count stays on the device
icpmi_status device_exclusive_scan_cursor(icpmi_ctx* c, unsigned* counts, unsigned* starts, int n, unsigned total, bool zero_counts, unsigned* tail_out = nullptr); // tail_out: receives counts[n + 1]
// the same scan on another stream with the caller's own chunk-total words (device_scan_side_words(n) of them); false from
// device_scan_side_ok(n): the table is too large for the two-kernel scan -- stay on the handle's stream
bool device_scan_side_ok(int n);
size_t device_scan_side_words(int n);
icpmi_status device_exclusive_scan_cursor_side(icpmi_ctx* c, hipStream_t stream, unsigned* sums, unsigned* counts, unsigned* starts, int n, unsigned total);
icpmi_status sort_queries(icpmi_ctx* c, const float4* d_pts, int64_t n);
icpmi_status sort_queries_reserve(icpmi_ctx* c, int64_t n, int nscan = 1);
icpmi_status sort_queries_batch(icpmi_ctx* c, const float4* d_pts, const BatchArgs& ba, const SortHead* head = nullptr); // slices of d_pts -> slices of d_qsorted / d_qindex
                                                                                 // (head: d_pts is WRITTEN first, from head->raw minus the mean)
// What ONE launch of the matcher is asked beyond the search itself, and what it answers.  The defaults are a stage call (icpmi_knn, the
// map-side operators): answers in the caller's order, no fused selection, unseeded, KDTreeMatcher's uniform radius, one reading.
struct NnRequest {
    unsigned*    hist0    = nullptr;   // build level 0 of the fused selection here if the launched variant can
    float4*      match_pt = nullptr;   // k = 1: keep the loop state (sidx, d2, matched point) in query order
    bool         sorted_k = false;     // k > 1: keep a query's k matches at its slot of the tile-sorted order
    const float* r2row    = nullptr;   // KDTreeVarDistMatcher / icpmi_knn_var: squared accept radii per query, caller's order (nn.hip: RowR2)
    int          iter     = 0;         // iteration index of this launch (> 0: seeded by the previous match)
    unsigned*    defer    = nullptr;   // k = 1, one reading, state in query order: far-seeded queries run in defer_wgs extra workgroups of eight
    int          defer_wgs = 0;        // (icpmi_ctx::d_defer and its layout; null = every query stays in its home workgroup)
    BatchArgs    batch{};              // nscan > 1: the readings of a batch (loop_run_batch); otherwise the launch's one reading of n points
};
struct NnOutcome {
    bool built_hist0 = false;          // the launched variant built level 0 of the fused selection
    bool built_win   = false;          // ... it counted the speculative window (ICPMI_S2_WIN: nnk_wg_kernel in a fused-selection loop)
    bool out_sorted  = false;          // the state it left is in query order (match_pt / sorted_k honoured)
};
icpmi_status nn_launch_k(icpmi_ctx* c, const NnRequest& req, const float4* d_reading, int64_t n, const float* d_T, const LoopCfg& lc,
                         int allow_self, int* d_sidx, float* d_d2, IcpState* d_state, NnOutcome* out = nullptr);
icpmi_status nn_ids_to_original(icpmi_ctx* c, const int* d_sidx, int64_t count, int* d_ids);
// select.hip: enqueue the quantile / scale selections chain lc needs over the `count` entries of c->d_d2 (no host sync); ba = the readings
// behind d_d2, nn = what the matcher's launch in front of it answered (the fused chain skips what that launch already built); legacy = the
// 11/11/10 passes even for a single quantile filter (no consumer kernel behind it to resolve a fused last level)
void enqueue_selection(icpmi_ctx* c, const LoopCfg& lc, int64_t count, const BatchArgs& ba, const NnOutcome& nn, bool legacy = false);
// ... and what those launches need allocated (a VarTrimmedDist chain's scratch), before a capture starts: enqueue_selection then cannot fail
icpmi_status selection_reserve(icpmi_ctx* c, const LoopCfg& lc, int64_t count);
// self k-NN of a device cloud through a sparse block grid built for the call (selfgrid.hip): rows of d_sidx / d_d2 in the cloud's order, entries =
// positions in c->d_map_sorted (w = original index bits), which the call leaves behind for launch_normals / nn_ids_to_original
// subset search of an appended cloud (selfgrid.hip): in -- m_old, d_dk (d^2 of the k-th neighbour of the first m_old points, original order);
// out -- d_list / n_sel: the searched original indices
struct SelfGridSubset { int64_t m_old = 0; const float* d_dk = nullptr; const unsigned* d_list = nullptr; int64_t n_sel = 0; };
icpmi_status selfgrid_knn(icpmi_ctx* c, const float4* d_pts, int64_t m, int k, int* d_sidx, float* d_d2, SelfGridSubset* sub = nullptr);
void selfgrid_destroy(icpmi_ctx* c);
icpmi_status selfgrid_debug_info(icpmi_ctx* c, uint64_t info[8]); // test seam: the grid of the handle's last selfgrid_knn
icpmi_status create_handle(const icpmi_config* cfg, icpmi_handle* out); // icpmi_create without the cache's handle count (private handles)
// d_r2row: the squared accept radii of a KDTreeVarDistMatcher registration (one per point of the reading), else nullptr
icpmi_status loop_run(icpmi_ctx* c, const float4* d_scan, const float* d_normals3, int64_t n, const LoopCfg& lc, const float* d_r2row, bool fixed,
                      float T_out[16], icpmi_stats* stats);
icpmi_status loop_sensor_noise_overlap(icpmi_ctx* c, int64_t n, const LoopCfg& lc, bool sorted, float* overlap);
icpmi_status loop_covariance(icpmi_ctx* c, int64_t n, const LoopCfg& lc, bool sorted);
const float* loop_covariance_out(const icpmi_ctx* c); // device address of the 36 floats loop_covariance leaves
icpmi_status loop_degen_stats(icpmi_ctx* c, int64_t n, const LoopCfg& lc);  // c0, L of the centred reading in c->d_reading -> lc.degen_blk (three launches)
icpmi_status loop_degen_report(icpmi_ctx* c, const LoopCfg& lc);            // the side block's last counted iteration -> its icpmi_localizability (one launch)
icpmi_status loop_prepare_reading(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_normals3, bool* head_done = nullptr);
icpmi_status loop_run_batch(icpmi_ctx* c, int batch, const float* const* d_scans4, const int64_t* n, const LoopCfg& lc, bool fixed,
                            float* T_out, icpmi_stats* stats, icpmi_status* status);
icpmi_status loop_single_step(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const float* T_iter_host, float T_step[16],
                              double sums[32], icpmi_stats* stats);
// VoxelMatcher (voxel.hip).  A handle runs it when the size is set and its minimiser is plane-to-plane with the GICP pair
// model; api.hip refuses every other combination before a loop starts
static inline bool voxel_path(const icpmi_ctx* c)
{
    return c->voxel_size > 0.f && c->cfg.minimizer == ICPMI_MIN_PLANE_TO_PLANE && c->plane_model == ICPMI_PLANE_MODEL_GICP;
}
// ... with a schedule of two or more levels: the pair kernel that reads the level, and the advance behind the solve
static inline bool voxel_scheduled(const icpmi_ctx* c) { return voxel_path(c) && c->vox_levels >= 2; }
// FNV-1a over n bytes, continued from h: what the signatures of captured loops are made of (loop.hip: loop_sig; voxel.hip: voxel_sched_sig)
static inline uint64_t fnv(const void* p, size_t n, uint64_t h)
{
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
uint64_t voxel_sched_sig(const icpmi_ctx* c, uint64_t h); // hash of what a captured voxel loop depends on, continued from h (0: a fresh one)
bool voxel_table_current(const icpmi_ctx* c);
icpmi_status voxel_ensure_table(icpmi_ctx* c, float* times_ms); // every level; times_ms (3 floats: sort, reduce, fill) forces a rebuild of the finest
void voxel_enqueue_pairs(icpmi_ctx* c, int64_t n, int nb, float eps); // one launch on c->stream: the sums of c->d_reading under d_state->T_iter
// (scheduled handles: the level word is set and raised by loop.hip's voxel_sched_reset_kernel and voxel_advance_kernel)
// A batch on the voxel path: the batch block (descriptors current, before anything is enqueued), the pair sums of one
// iteration of all members (blockIdx.y = member; nb = acc_blocks of the largest, cap = the cap of acc_blocks), and the loop: B readings
// with their normals (3 floats per point, device) registered in one loop, every member to the bits loop_run gives it alone
icpmi_status voxel_ensure_batch_block(icpmi_ctx* c);
void voxel_enqueue_pairs_batch(icpmi_ctx* c, const BatchArgs& ba, int nb, int cap, float eps);
icpmi_status loop_run_voxel_batch(icpmi_ctx* c, int batch, const float* const* d_scans4, const int64_t* n, const float* const* d_normals3,
                                  const LoopCfg& lc, float* T_out, icpmi_stats* stats, icpmi_status* status);
icpmi_status voxel_get_map(icpmi_ctx* c, int level, int64_t cap, int32_t* ijk3, float* mean3, float* moments6, int32_t* count, int64_t* n_voxels);
icpmi_status voxel_lookup(icpmi_ctx* c, int level, const float* q4_centred, int64_t n, int32_t* voxel);
icpmi_status voxel_lookup_times(icpmi_ctx* c, const float* q4_centred, int64_t n, int reps, float ms[2], int64_t* mismatch); // table against binary search
// icpmi_voxel_score_poses* (DESIGN.md 4.22): the raw reading d_scan / d_n3 under n_poses centred-frame poses (16 floats each), scored against
// level `level`'s table (current: voxel_ensure_table); out[p] complete, hb = 0.5f * beta.  loop_centre_pad (loop.hip) prepares the reading
icpmi_status voxel_score_poses(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_n3, const float* Tc, int n_poses, int level, float hb,
                               icpmi_voxel_score* out);
void voxel_score_shape(int32_t* slice, int32_t* tile);
// Global localisation (occupancy.hip).  occ_ensure: the pyramid of the resident map for (s0, levels), built unless current.
// occ_get_level: the keys of occB_level as cells, ascending.  occ_score_nodes: bound(k, l, A) of n_nodes caller-checked nodes (5 ints each)
// for the raw reading d_scan under the n_rot rotations R9 (host, 9 floats each, column-major).  occ_global_localize: the search over the
// window [a_min, a_max] with `levels` levels; every argument is checked by the caller (api.hip), the result arrives zeroed.
icpmi_status occ_ensure(icpmi_ctx* c, float s0, int levels);
icpmi_status occ_get_level(icpmi_ctx* c, float s0, int levels, int level, int64_t cap, int32_t* ijk3, int64_t* n_keys);
icpmi_status occ_score_nodes(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* R9, int n_rot, float s0, int levels, const int32_t* nodes5,
                             int64_t n_nodes, int64_t* counts);
icpmi_status occ_global_localize(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* R9, int n_rot, float s0, int levels, const int64_t a_min[3],
                                 const int64_t a_max[3], int batch, int64_t need, int64_t max_nodes, icpmi_global_localize_result* res);
void occ_shape(int32_t* slice, int32_t* tile, int32_t* launch_nodes);
icpmi_status loop_centre_pad(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_normals3, float4* d_pts, float4* d_nrm);
// the reading's normals (host, 3 per point) into c->d_read_normals, padded as a registration's head pads them
icpmi_status loop_upload_read_normals(icpmi_ctx* c, const float* normals3, int64_t n);
// getResidualError() of the centred reading in c->d_reading under the centred-frame pose T (host, column-major); kind 1 / 2
icpmi_status loop_residual(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const float T[16], int kind, int planar, const float* d_r2row,
                           icpmi_residual* out);
// ... of the raw reading d_scan under n_poses centred-frame poses (16 floats each) through batched launches (blockIdx.y = pose); centres and
// sorts the reading itself, once.  out[p] arrives initialised; status[p] = what loop_residual would return for pose p
icpmi_status loop_residual_poses(icpmi_ctx* c, const float4* d_scan, int64_t n, const LoopCfg& lc, const float* T, int n_poses, int kind, int planar,
                                 icpmi_residual* out, icpmi_status* status);
icpmi_status loop_outlier_weights(icpmi_ctx* c, const LoopCfg& lc, const float* d2, const int32_t* ids, int k, int64_t n,
                                  const float* read_normals3, float* weights, float* limit_out);
// the one-pass front of loop_residual, shared with sweep.hip (each is described where loop.hip defines it): the loop's buffers, fresh
// states, the chain as one pass, what that pass asks of the matcher, the matcher's launch + the selections, and the view of what they leave
icpmi_status ensure_loop_buffers(icpmi_ctx* c, int64_t n, const LoopCfg& lc, int nscan = 1);
icpmi_status enqueue_fresh_states(icpmi_ctx* c, int nstates, const float* d_T0);
LoopCfg one_pass_cfg(const LoopCfg& lc);
NnRequest loop_request(icpmi_ctx* c, const LoopCfg& lc, const BatchArgs& ba, const float* d_r2row);
icpmi_status enqueue_match_select(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const NnRequest& req, NnOutcome* nn, hipEvent_t matched = nullptr);
PairView pair_view(const icpmi_ctx* c, const LoopCfg& lc, bool sorted);
LoopCfg make_loop_cfg(const icpmi_ctx* c, int fixed_iterations);
// How a call over many items (the readings of a batch, the starts of a multistart, the poses of a residual call) ends: per_item goes to
// status_out when the caller took that array, and the call then returns OK; otherwise it returns the first error.  text: what last_error
// says when an item failed (null: the failed item's own words stay)
static inline icpmi_status fold_status(icpmi_ctx* c, icpmi_status* status_out, const icpmi_status* per_item, int count, const char* text)
{
    icpmi_status first = ICPMI_OK;
    for (int i = 0; i < count; ++i) {
        if (status_out) status_out[i] = per_item[i];
        if (per_item[i] != ICPMI_OK && first == ICPMI_OK) first = per_item[i];
    }
    if (first != ICPMI_OK && text) c->last_error = text;
    return status_out ? ICPMI_OK : first;
}

// ---- shared by the operator files: pointops.hip (a caller's cloud), dynpts.hip (DynamicPoints), ops.hip (the resident map) ----
// A 4 x 4 (col-major) as a kernel ARGUMENT: the matrix rides in the kernarg segment (scalar loads), no device copy of it and no upload
// launch in front of the kernel that reads it (r5: the map-update chain uploaded four matrices per update, one copy kernel each).
struct Mat16 { float v[16]; };
static inline Mat16 mat16(const float T[16]) { Mat16 m; memcpy(m.v, T, sizeof m.v); return m; }
// `dists(i) >= std::pow(minDistNewPoint, 2)` (PointDistanceMapperModule.cpp:42): std::pow(float, int) is evaluated in
// double and the float distance is promoted for the comparison.  The product of two floats is exact in double.
inline double pd_limit(float min_dist) { return (double)min_dist * (double)min_dist; }
// squared search radius that is guaranteed to return every neighbour with d2 < limit (the smallest float >= limit)
inline float pd_radius2(double lim) { float r = (float)lim; if ((double)r < lim) r = nextafterf(r, INFINITY); return r; }
// helper: a private handle on the same device/stream used to index an arbitrary cloud without
// disturbing the ICP map of the caller's handle
// The private handle lives as long as its owner (created on first use, destroyed by icpmi_destroy): its buffers are
// reused from call to call instead of ~20 hipMalloc / hipFree pairs per operator call.
struct TempCtx {
    icpmi_handle h = nullptr;
};
icpmi_status make_temp(icpmi_ctx* c, TempCtx& t);
void share_stream(icpmi_ctx* c, icpmi_ctx* t); // the private handle t enqueues on its owner's stream from here on
icpmi_status check_rigid(icpmi_ctx* c, const float T[16]); // Transformation::checkParameters
void launch_normals(hipStream_t stream, const float4* map, const int* sidx, int64_t m, int k, float* normals3, float* densities, int dim2,
                    float* mean_dist = nullptr, float* eig_values = nullptr, float* eig_vectors = nullptr, const unsigned* list = nullptr);
template <typename T> // uint8_t (a host mask) or unsigned (device compaction): instantiated in pointops.hip
icpmi_status voxel_flags_dev(icpmi_ctx* c, const float4* d_in, int64_t n, float edge, int method, T* d_keep);
icpmi_status ops_move_dev(icpmi_ctx* c, const float T[16], float4* d_pts, float* d_n3, int64_t m);
icpmi_status dynpts_dev(icpmi_ctx* c, const icpmi_dynpts_params* prm, const float T[16], const float4* d_in, int64_t n,
                        const float4* d_map, const float* d_nrm, int64_t m, float* d_prob, hipStream_t stream);
bool dynpts_side_ok(const icpmi_dynpts_params* prm);
icpmi_status dynpts_check(icpmi_ctx* c, const icpmi_dynpts_params* prm); // ICPMI_ERR_UNSUPPORTED: a half angle whose angular grid is too large

icpmi_status ops_transform(icpmi_ctx* c, const float T[16], const float* in4, int64_t n, float* out4,
                           const float* in_n3, float* out_n3);
icpmi_status ops_map_update_chain(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_scan_n3, const float* d_scan_s,
                                  const float to_sensor[16], const float from_sensor[16], const icpmi_map_op* ops, int n_ops, int n_modules,
                                  int32_t* src_out, int64_t src_capacity, int64_t* identity_prefix, int64_t* new_m);
#define ICPMI_MAX_POINT_FILTERS 16
icpmi_status ops_filter_points(icpmi_ctx* c, const float* in4, int64_t n, const icpmi_point_filter* filters, int n_filters, uint8_t* keep);
#define ICPMI_MAX_SENSOR_STEPS 8
icpmi_status ops_sensor_model(icpmi_ctx* c, const float* in4, int64_t n, const float* normals3_in, const float* obs_dir3_in, const icpmi_sensor_step* steps,
                              int n_steps, float* normals3_out, float* obs_dir3_out, float* noise_out, uint8_t* keep_out);
icpmi_status ops_staged_keep(icpmi_ctx* c, const float correction[16], float min_dist, uint8_t* keep_out, float* placed_out4);
icpmi_status ops_map_scalar(icpmi_ctx* c, const float* set, float* get, int64_t m);
icpmi_status ops_get_map_densities(icpmi_ctx* c, float* out, int64_t capacity);
bool max_density_param_ok(float max_density); // finite and > 0
icpmi_status max_density_flags_dev(icpmi_ctx* c, const float* d_dens, int64_t n, float max_density, int seed, unsigned* d_flag, unsigned* d_rank);
icpmi_status ops_max_density_keep(icpmi_ctx* c, const float* densities, int64_t n, float max_density, int seed, uint8_t* keep);
icpmi_status ops_surface_normals(icpmi_ctx* c, const float* pts4, int64_t m, int knn, float* normals3, float* densities = nullptr,
                                 int32_t* matched_ids = nullptr, float* mean_dist = nullptr, float* eig_values = nullptr, float* eig_vectors = nullptr);
// pointops.hip: the intensity gradients of a cloud with normals (host pointers), and the resident map's (g, I) channel from the caller's row
icpmi_status ops_intensity_gradient(icpmi_ctx* c, const float* pts4, int64_t m, const float* normals3, const float* intensity, int knn, float* grad3);
icpmi_status ops_set_map_intensity(icpmi_ctx* c, const float* intensity, int64_t m, int knn);
// test seams (icpmi_debug_self_knn / icpmi_debug_resident_kth_d2)
icpmi_status ops_debug_self_knn(icpmi_ctx* c, const float* pts4, int64_t m, int k, int32_t* ids, float* d2, uint64_t* info);
icpmi_status ops_debug_resident_kth_d2(icpmi_ctx* c, int64_t m, float* out, int32_t* knn_out);
icpmi_status ops_debug_merge_blocks(icpmi_ctx* c, const float* pts4, const int64_t* counts, int n_ranks, int64_t stride, float min_dist, int mode,
                                    float* merged_out4, int64_t capacity, int64_t* merged_n, uint8_t* kept_out, int32_t* path_out);
icpmi_status ops_dynamic_points_update(icpmi_ctx* c, const icpmi_dynpts_params* prm, const float to_sensor[16], const float* in4, int64_t n,
                                       const float* map4, const float* map_normals3, int64_t m, float* prob);
icpmi_status ops_map_update_point_distance(icpmi_ctx* c, const float* scan4, int64_t n, const float* scan_normals3, float min_dist,
                                           int normals_knn, uint8_t* keep_out, int64_t* appended, int64_t* new_m);
icpmi_status ops_map_update_dev(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_scan_n3, float min_dist, int normals_knn,
                                uint8_t* keep_out, int64_t* appended, int64_t* new_m);
icpmi_status ops_transform_dev(icpmi_ctx* c, const float T[16], const float4* d_in, int64_t n, float4* d_out);
icpmi_status ops_transform_normals_dev(icpmi_ctx* c, const float T[16], const float4* d_in, const float* d_in3, int64_t n, float4* d_out, float* d_out3);
icpmi_status ops_get_map(icpmi_ctx* c, float* out4, float* normals3, int64_t capacity, int64_t* m);
icpmi_status ops_voxel_keep_first(icpmi_ctx* c, const float* in4, int64_t n, float edge, int method, uint8_t* keep);
icpmi_status ops_point_distance_keep(icpmi_ctx* c, const float* map4, int64_t m, const float* in4, int64_t n,
                                     float min_dist, uint8_t* keep);
icpmi_status ops_bin_cells(icpmi_ctx* c, const float* pts4, int64_t n, float cell_size, int32_t* ijk3);
icpmi_status comm_unique_id(icpmi_comm_id* id, std::string& err);
icpmi_status comm_init(icpmi_ctx* c, const icpmi_comm_id* id, int n_ranks, int rank);
icpmi_status comm_destroy(icpmi_ctx* c);
icpmi_status comm_info(icpmi_ctx* c, int* n_ranks, int* rank, int* kind);
icpmi_status comm_allgather(icpmi_ctx* c, const void* d_send, void* d_recv, size_t count, bool is_float);
// all-gather of one fixed-size block of `block4` float4 per rank (element 0 = header: x = bits(count) or bits(-1)); the loopback
// communicator builds its simulated ranks' blocks (shifted points, ragged counts) in one launch.  No communicator: d_recv = a copy of d_send.
icpmi_status comm_allgather_blocks(icpmi_ctx* c, const float4* d_send, float4* d_recv, size_t block4);
icpmi_status merge_blocks_reserve(icpmi_ctx* c, int n_ranks); // the exchange buffers of the one-collective epoch (called by comm_init)
icpmi_status ops_staged_merge_allgather(icpmi_ctx* c, const float correction[16], float min_dist, int normals_knn, int64_t* accepted_local,
                                        int64_t* appended_total, int64_t* new_m, float* merged_out4, int64_t merged_capacity, int64_t* merged_n);
icpmi_status ops_staged_merged_points(icpmi_ctx* c, float* out4, int64_t capacity, int64_t* n);
icpmi_status ops_staged_bin_cells(icpmi_ctx* c, float cell_size, int32_t* ijk3, int64_t* offsets, int64_t* counts, int64_t capacity, int64_t* n_cells);
icpmi_status ops_cell_log_read(icpmi_ctx* c, int64_t offset, int64_t count, float* out4, int64_t* log_size);
icpmi_status ops_cell_log_clear(icpmi_ctx* c);
icpmi_status ops_cells_enqueue_in_epoch(icpmi_ctx* c);
icpmi_status ssn_debug_minstd(icpmi_ctx* c, unsigned seed, unsigned n, unsigned* out);
icpmi_status ssn_sample_dev(icpmi_ctx* c, const float4* d_in, int64_t n, float ratio, int knn, float max_box, unsigned seed, int* d_order_out,
                            float* d_normals_out, int64_t* n_out, int method = 0, float* d_mean_out = nullptr, int* d_mstart_out = nullptr,
                            int* d_mcount_out = nullptr, int* d_members_out = nullptr, int64_t* n_members_out = nullptr);
icpmi_status ops_sampling_surface_normal_ex(icpmi_ctx* c, const float* in4, int64_t n, float ratio, int knn, float max_box, int seed, int method,
                                            int32_t* order_out, float* normals3_out, int64_t* n_out, float* mean3_out, int32_t* mstart_out,
                                            int32_t* mcount_out, int32_t* members_out);
icpmi_status ops_sampling_surface_normal(icpmi_ctx* c, const float* in4, int64_t n, float ratio, int knn, float max_box, int seed, int32_t* order_out,
                                         float* normals3_out, int64_t* n_out);
size_t radix_sort_tab_words(int64_t n, int bits);
icpmi_status radix_sort_pairs(icpmi_ctx* c, unsigned long long* d_keys2, unsigned* d_vals2, int64_t n, int bits, unsigned* d_tab, int* result_half);
icpmi_status octree_sample_dev(icpmi_ctx* c, const float4* d_in, int64_t n, float max_size, int max_pts, int method, int* d_order, int* d_leaf_of,
                               int64_t* n_out);
icpmi_status ops_octree_sample(icpmi_ctx* c, const float* in4, int64_t n, float max_size, int max_pts, int method, int32_t* order_out,
                               int32_t* leaf_of_out, int64_t* n_out);
icpmi_status ops_voxel_grid(icpmi_ctx* c, const float* in4, int64_t n, const float vsize[3], int average, const float* desc, int rows,
                            int32_t* order_out, float* out4, float* desc_out, int64_t* n_out);
icpmi_status ops_covariance_sampling(icpmi_ctx* c, const float* in4, int64_t n, const float* normals3, int64_t nb, int torque_norm, int32_t* order_out,
                                     icpmi_covsamp_info* info_out);
icpmi_status ops_normal_space_sampling(icpmi_ctx* c, const float* in4, int64_t n, const float* normals3, int64_t nb, unsigned seed, float eps,
                                       int32_t* order_out, int32_t* bucket_out);
// deskew.hip: the table of icpmi_deskew_table (host, no device call), and icpmi_deskew (dev == false) / icpmi_deskew_dev (dev == true)
icpmi_status deskew_table_host(const icpmi_sweep_motion* m, float* q4, float* p3, float* omega, float* inv_sin, std::string& err);
icpmi_status ops_deskew(icpmi_ctx* c, const float* in4, int64_t n, const float* t_rel, const icpmi_sweep_motion* m, float* out4,
                        const float* in_normals3, float* out_normals3, bool dev);
// ... and the kernel alone on device pointers, no wait for its error flag (the caller has checked the point times; deskew.hip has the rules)
icpmi_status deskew_enqueue_dev(icpmi_ctx* c, const float4* d_in, int64_t n, const float* d_t_rel, const icpmi_sweep_motion* m, unsigned char* d_tab,
                                float4* d_out);
// sweep.hip: sweep registration (include/icpmi.h: icpmi_register_sweep has the formulation).  d_scan / d_t_rel: the raw scan and its point
// times on the device; lc: the chain as chain_setup built it.  sweep_sums_dev: steps 1 to 4 once under the given poses (column-major 4 x 4);
// sweep_register_dev: the iteration; d_out4 (may be null): the scan deskewed to the end pose under the final motion
icpmi_status sweep_sums_dev(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_t_rel, const LoopCfg& lc, const float* d_r2row,
                            const float T_begin[16], const float T_end[16], const icpmi_sweep_options* opts, double sums[80], icpmi_sweep_result* res);
icpmi_status sweep_register_dev(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_t_rel, const LoopCfg& lc, const float* d_r2row,
                                const float T_begin[16], const float T_end[16], const icpmi_sweep_options* opts, icpmi_sweep_result* res, float4* d_out4);
icpmi_status sweep_check_options(const icpmi_sweep_options* opts, std::string& err);
void sweep_result_priors(const float T_begin[16], const float T_end[16], icpmi_sweep_result* res);
icpmi_status sweep_solve_host(const double sums[80], double lambda_rot, double lambda_trans, const double* d6, double x12[12], std::string& err);

// ---- shared by the passes over the matcher's output: loop.hip (overlap, covariance, residual) and sweep.hip (the sweep's pair sums) ----
// ---------------------------------------------------------------------------------------------
// outlier weight of one match (OutlierFilters::compute; weights multiply)
// ---------------------------------------------------------------------------------------------
// M-estimator weight of RobustOutlierFilter for the scaled squared residual e2 (tuning k); exp / pow through double so that
// host libm and device ocml round to the same float
__device__ __forceinline__ float robust_weight(int fct, float e2, float kk)
{
    const float k2 = kk * kk;
    float w;
    switch (fct) {
    case ICPMI_ROB_CAUCHY: w = 1.f / (1.f + e2 / k2); break;
    case ICPMI_ROB_WELSCH: w = (float)exp((double)(-e2 / k2)); break;
    case ICPMI_ROB_SC: { const float t = kk + e2; w = e2 >= kk ? 4.f * k2 * (1.f / (t * t)) : 1.f; break; }
    case ICPMI_ROB_GM: { const float t = kk + e2; w = k2 * (1.f / (t * t)); break; }
    case ICPMI_ROB_TUKEY: { const float t = 1.f - e2 / k2; w = e2 >= k2 ? 0.f : t * t; break; }
    case ICPMI_ROB_HUBER: w = e2 >= k2 ? kk * (1.f / sqrtf(e2)) : 1.f; break;
    case ICPMI_ROB_L1: w = 1.f / sqrtf(e2); break;
    default: {
        const float pw = (float)pow((double)(1.f + e2 / kk), (double)(-(kk + 3.f) / 2.f));
        w = pw * (kk + 3.f) * (1.f / (kk + e2));
        break; }
    }
    return w <= 0.f ? 0.f : w;
}

// EXT: chains with GenericDescriptor / Robust filters -- ref_scalar (per ORIGINAL map index `orig`) and the squared
// point-to-plane distance of the pair (plane2) come from the caller
template <bool EXT = false>
__device__ __forceinline__ float match_weight(const LoopCfg& lc, const IcpState* __restrict__ st, float d2,
                                              const float* __restrict__ T, const float4* __restrict__ read_normals, int qi,
                                              const float4* __restrict__ ref_normals, int sidx, int fused_slot = -1,
                                              float fused_limit = 0.f, const float* __restrict__ ref_scalar = nullptr, int orig = 0,
                                              float plane2 = 0.f, const float4* rn_kept = nullptr)
{
    float w = 1.f;
    for (int f = 0; f < lc.n_out; ++f) {
        const int type = lc.out_type[f];
        const float prm = lc.out_param[f];
        if (type == ICPMI_OUT_MAXDIST) w *= (d2 <= prm * prm) ? 1.f : 0.f;
        else if (type == ICPMI_OUT_MINDIST) w *= (d2 >= prm * prm) ? 1.f : 0.f;
        else if (type == ICPMI_OUT_MEDIANDIST || type == ICPMI_OUT_TRIMMEDDIST || type == ICPMI_OUT_VARTRIMMEDDIST)
            w *= (d2 <= (f == fused_slot ? fused_limit : st->limits[f])) ? 1.f : 0.f;
        else if (type == ICPMI_OUT_SURFACENORMAL) {
            const float4 a = rn_kept ? *rn_kept : read_normals[qi]; // (rn_kept: the plane-to-plane pair sums hold the reading's normal already)
            float ax = a.x, ay = a.y, az = a.z;
            if (T) { // descriptors named "normals" rotate with the cloud
                const float rx = fmaf(T[8], az, fmaf(T[4], ay, T[0] * ax));
                const float ry = fmaf(T[9], az, fmaf(T[5], ay, T[1] * ax));
                const float rz = fmaf(T[10], az, fmaf(T[6], ay, T[2] * ax));
                ax = rx; ay = ry; az = rz;
            }
            const float4 b = ref_normals[sidx];
            const float dot = fmaf(az, b.z, fmaf(ay, b.y, ax * b.x));
            w *= (dot > cosf(prm)) ? 1.f : 0.f;
        } else if (EXT && type == ICPMI_OUT_GENERICDESCRIPTOR) {
            const int ip = lc.out_iparam[f];
            const float v = (ip & ICPMI_GEN_SOURCE_READING) ? lc.read_scalar[qi] : ref_scalar[orig];
            w *= (ip & ICPMI_GEN_SOFT) ? v : ((ip & ICPMI_GEN_LARGER) ? (v > prm ? 1.f : 0.f) : (v < prm ? 1.f : 0.f));
        } else if (EXT && type == ICPMI_OUT_ROBUST) {
            const int ip = lc.out_iparam[f];
            const int se = (ip >> 4) & 15, fct = ip & 15;
            const float sc = se != ICPMI_SCALE_NONE ? st->robust_scale : 1.f;
            const float res = ((ip >> 8) & 15) == ICPMI_DIST_POINT2PLANE ? plane2 : d2;
            // berg: `tuning` is the scale the estimate converges to; the M-estimator runs on Bergstrom's constants
            const float kk = se != ICPMI_SCALE_BERG ? prm : (fct == ICPMI_ROB_CAUCHY ? 4.3040f : fct == ICPMI_ROB_TUKEY ? 7.0589f : fct == ICPMI_ROB_HUBER ? 2.0138f : prm);
            const float e2 = res / (sc * sc);
            const float apx = lc.out_param3[f];
            float rw = robust_weight(fct, e2, kk);
            if (apx > 0.f && apx != INFINITY && e2 >= apx * apx) rw = 0.f;
            w *= rw;
        }
    }
    return w;
}

// ---------------------------------------------------------------------------------------------
// The pair sums of the iteration: what loop.hip's accumulate_kernel and voxel.hip's voxel_pairs_kernel add per pair, and how a workgroup's
// sums join the iteration's accumulator.  Per-pair terms in float without contraction, the weight's products and the sums in double.
// ---------------------------------------------------------------------------------------------
// a normal scaled to length 1; a zero or non-finite one is "no surface model" (zero: that side's covariance becomes I)
__device__ __forceinline__ float3 unit_or_zero(float x, float y, float z)
{
    const float l2 = x * x + y * y + z * z;
    const bool ok = l2 > 0.f && l2 < INFINITY;
    const float inv = ok ? 1.f / sqrtf(l2) : 0.f;
    return ok ? make_float3(x * inv, y * inv, z * inv) : make_float3(0.f, 0.f, 0.f);
}
__device__ __forceinline__ float3 cross3(float3 a, float3 b) { return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// generalized ICP: A += w G M G^T, b -= w G M d with G = J^T = [[p]x; I], M = S^-1, S = the sum of the pair's two
// covariances (symmetric: xx xy xz yy yz zz), d = p - q.  M = n n^T would give the point-to-plane sums: G n = F.  WEIGHTED = false: weight 1, and
// no multiplication by it.  Every group joins its sums as soon as it exists: the live floats of a pair stay few.
template <bool WEIGHTED>
__device__ __forceinline__ void gicp_pair_sums(double (&acc)[27], float sxx, float sxy, float sxz, float syy, float syz, float szz, float3 p, float3 d,
                                               double dw)
{
    auto wt = [&](float v) { return WEIGHTED ? dw * v : (double)v; };
    // M = adj(S) / det(S)
    const float c00 = syy * szz - syz * syz, c01 = sxz * syz - sxy * szz, c02 = sxy * syz - sxz * syy;
    const float c11 = sxx * szz - sxz * sxz, c12 = sxy * sxz - sxx * syz, c22 = sxx * syy - sxy * sxy;
    const float idet = 1.f / (sxx * c00 + sxy * c01 + sxz * c02);
    const float3 m0 = make_float3(c00 * idet, c01 * idet, c02 * idet), m1 = make_float3(m0.y, c11 * idet, c12 * idet),
                 m2 = make_float3(m0.z, m1.z, c22 * idet);
    acc[15] += wt(m0.x); acc[16] += wt(m0.y); acc[17] += wt(m0.z); acc[18] += wt(m1.y); acc[19] += wt(m1.z); acc[20] += wt(m2.z);
    const float3 md = make_float3(m0.x * d.x + m0.y * d.y + m0.z * d.z, m1.x * d.x + m1.y * d.y + m1.z * d.z, m2.x * d.x + m2.y * d.y + m2.z * d.z);
    const float3 pmd = cross3(p, md);
    acc[21] -= wt(pmd.x); acc[22] -= wt(pmd.y); acc[23] -= wt(pmd.z); acc[24] -= wt(md.x); acc[25] -= wt(md.y); acc[26] -= wt(md.z);
    // P M with P = [p]x: column j is p x (column j of M); row i of P M P^T is p x (row i of P M)
    const float3 k0 = cross3(p, m0), k1 = cross3(p, m1), k2 = cross3(p, m2);
    const float3 pm0 = make_float3(k0.x, k1.x, k2.x), pm1 = make_float3(k0.y, k1.y, k2.y), pm2 = make_float3(k0.z, k1.z, k2.z);
    acc[3] += wt(pm0.x); acc[4] += wt(pm0.y); acc[5] += wt(pm0.z);
    acc[8] += wt(pm1.x); acc[9] += wt(pm1.y); acc[10] += wt(pm1.z);
    acc[12] += wt(pm2.x); acc[13] += wt(pm2.y); acc[14] += wt(pm2.z);
    const float3 r0 = cross3(p, pm0), r1 = cross3(p, pm1), r2 = cross3(p, pm2);
    acc[0] += wt(r0.x); acc[1] += wt(r0.y); acc[2] += wt(r0.z); acc[6] += wt(r1.y); acc[7] += wt(r1.z); acc[11] += wt(r2.z);
}

// The workgroup's sums (BT threads; acc: the NVAL values of the model, then sum w and the pair count, EXT: force2D's b, else b2d is not
// read) join the iteration's accumulator at hists + ICPMI_S2_ACC.  Lane exchanges in registers (lane_xor), then LDS across the waves.
// Transposed butterfly: at the step with partner lane ^ m every lane hands over the half of its values the partner keeps, so 32 values x
// 64 lanes fold with 16+8+4+2+1+1 = 32 exchanges instead of 32 x 6.  After the five halving steps lane l holds value bitrev5(l & 31)
// summed over its 32-lane half; the last exchange joins the halves.  Fixed pattern => deterministic sums.
// (voxel.hip's caller.  loop.hip's accumulate_kernel keeps the same fold spelled out in its body, value for value: see there.)
template <int BT, int NVAL, bool EXT>
__device__ __forceinline__ void pair_sums_fold(const double (&acc)[NVAL > 0 ? NVAL : 1], double wsum, double cnt, const double* b2d, unsigned* hists)
{
    __shared__ double sh[BT / 64][ICPMI_NV];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double val[ICPMI_NV];
#pragma unroll
    for (int i = 0; i < ICPMI_NV; ++i) val[i] = i < NVAL ? acc[i < NVAL ? i : 0] : 0.0;
    val[27] = wsum; val[28] = cnt;
    if constexpr (EXT) { val[29] = b2d[0]; val[30] = b2d[1]; val[31] = b2d[2]; }
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int m = 1 << s;
        const int nkeep = 16 >> s;
        const bool upper = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < nkeep; ++i) {
            const double send = upper ? val[i] : val[i + nkeep];
            const double keep = upper ? val[i + nkeep] : val[i];
            val[i] = keep + lane_xor_bit(send, m); // (the partner is lane ^ m, as with __shfl_xor: the same tree of additions)
        }
    }
    val[0] += lane_xor<32>(val[0]);
    if (lane < 32) {
        const int idx = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
        sh[wv][idx] = val[0];
    }
    __syncthreads();
    if (threadIdx.x < ICPMI_NV) {
        const int i = threadIdx.x;
        double v = 0.0;
        if (i < NVAL || i == 27 || i == 28 || (EXT && i > 28)) {
            v = sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i];
#pragma unroll
            for (int w2 = 4; w2 < BT / 64; ++w2) v += sh[w2][i]; // fixed order
        }
        // the workgroup's sum joins the iteration's accumulator as two fixed-point limbs (ICPMI_ACC_*): integer atomics, so the total is
        // the same whatever order the workgroups arrive in
        unsigned long long* out = reinterpret_cast<unsigned long long*>(hists + ICPMI_S2_ACC);
        if (v != 0.0) {
            if (!(fabs(v) < 0x1p77)) atomicOr(reinterpret_cast<unsigned*>(out + ICPMI_ACC_FLAG), 1u);
            else {
                const double hi = rint(v * 0x1p-16);
                const double lo = v - hi * 65536.0;                 // exact: a multiple of ulp(v) below 2^15
                const long long H = (long long)hi, Lq = __double2ll_rn(lo * 0x1p40);
                const int cp = blockIdx.x & (ICPMI_ACC_COPIES - 1);
                if (H) atomicAdd(out + ICPMI_ACC_IDX(cp, i, 0), (unsigned long long)H);
                if (Lq) atomicAdd(out + ICPMI_ACC_IDX(cp, i, 1), (unsigned long long)Lq);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The passes over the matcher's output OUTSIDE the iteration (overlap, covariance, residual) share one walk and one way to sum.
// ---------------------------------------------------------------------------------------------
// one live slot (d2 finite) as walk_pairs hands it to a pass: p = the reading's point under T, q = its match, (dx, dy, dz) = p - q in
// float as the pair-sum kernel forms it, nm / dot = the match's normal and (p - q) . nm (zero without map normals), w = the chain's weight
struct PairSlot { int64_t e; int qi, oi, s; float d2; float3 p; float4 q, nm; float dx, dy, dz, dot, w; };

// slice blockIdx.y of the per-query arrays (a pose batch: common.h, BatchArgs); the reading's descriptors are not sliced
__device__ __forceinline__ void pair_view_slice(PairView& v, const BatchArgs& ba, int k)
{
    const size_t qo = (size_t)blockIdx.y * (size_t)ba.qstride;
    v.reading += qo; v.sidx += qo * k; v.d2 += qo * k;
    if (v.qindex) v.qindex += qo;
    if (v.match_pt) v.match_pt += qo;
}

// Grid-stride walk of the n * lc.k slots by 256-thread workgroups; body(slot) runs for every slot with a match.  The weight goes to the
// body as it is: each pass has its own acceptance test.  fused_slot / fused_limit: match_weight's (a limit the caller resolved itself).
template <class Body>
__device__ __forceinline__ void walk_pairs(const PairView& v, int n, const LoopCfg& lc, const IcpState* __restrict__ st,
                                           const float* __restrict__ T, Body body, int fused_slot = -1, float fused_limit = 0.f)
{
    const int64_t total = (int64_t)n * lc.k;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        PairSlot a;
        a.d2 = v.d2[e];
        if (a.d2 == INFINITY) continue;
        a.e = e;
        a.qi = (int)(e / lc.k);
        a.oi = v.qindex ? v.qindex[a.qi] : a.qi;
        a.s = v.sidx[e];
        // the three gathers of a pair are requested together, in front of the first use of any of them (with k > 1 the matched point and
        // its normal both hang on s: a normal fetched behind p - q is one more round trip per pair, 2 us of a knn-6 pass)
        const float4 r = v.reading[a.qi];
        a.q = v.match_pt ? v.match_pt[e] : v.map[a.s];
        a.nm = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v.ref_normals) a.nm = v.ref_normals[a.s];
        a.p = xf_point(T, r.x, r.y, r.z, r.w);
        a.dx = a.p.x - a.q.x; a.dy = a.p.y - a.q.y; a.dz = a.p.z - a.q.z;
        a.dot = v.ref_normals ? a.dx * a.nm.x + a.dy * a.nm.y + a.dz * a.nm.z : 0.f;
        // EXT: the filters that read the pair itself, as the pair-sum kernel evaluates them
        if (lc.ext) a.w = match_weight<true>(lc, st, a.d2, T, v.read_normals, a.oi, v.ref_normals, a.s, fused_slot, fused_limit, v.ref_scalar,
                                             __float_as_int(a.q.w), a.dot * a.dot);
        else a.w = match_weight(lc, st, a.d2, T, v.read_normals, a.oi, v.ref_normals, a.s, fused_slot, fused_limit);
        body(a);
    }
}

// Ordered double sums: a fixed pattern at every level, so a pass gives the same bits on every call (include/icpmi.h rests on it).
// Level 1, all 256 threads: acc[NV] per thread -> xor butterfly 32 .. 1 inside the wave -> the four waves in order -> row[NV], this
// workgroup's row of partials.  Slots whose bit is set in MAXMASK combine with fmax instead of +.
template <int NV, unsigned MAXMASK = 0u>
__device__ __forceinline__ void block_partial_row(const double (&acc)[NV], double* __restrict__ row)
{
    __shared__ double sh[4][NV];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double v = acc[i];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const double o = lane_xor_bit(v, m);
            v = (MAXMASK >> i & 1u) ? fmax(v, o) : v + o;
        }
        if (lane == 0) sh[wv][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int i = threadIdx.x;
        row[i] = (MAXMASK >> i & 1u) ? fmax(fmax(fmax(sh[0][i], sh[1][i]), sh[2][i]), sh[3][i]) : ((sh[0][i] + sh[1][i]) + sh[2][i]) + sh[3][i];
    }
}

// Level 2, one workgroup of at least NV * CH threads: the first nb <= NB rows -> tot[NV] (LDS, valid in every thread on return).  Thread
// v * CH + ch adds rows ch, ch + CH, ... of value v in that order -- every load issued before the first add (a loop of dependent loads and
// adds was 35 us at 128 rows) -- and thread v then adds the CH chunk sums in order.
template <int NV, int CH, int NB, unsigned MAXMASK = 0u>
__device__ __forceinline__ void block_ordered_total(const double* __restrict__ partial, int nb, double* tot)
{
    __shared__ double part[NV][CH];
    if (threadIdx.x < NV * CH) {
        constexpr int PER = (NB + CH - 1) / CH;
        const int v = threadIdx.x / CH, ch = threadIdx.x % CH;
        double x[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int b = ch + CH * i;
            x[i] = b < nb ? partial[(size_t)b * NV + v] : 0.0;
        }
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < PER; ++i) acc = (MAXMASK >> v & 1u) ? fmax(acc, x[i]) : acc + x[i];
        part[v][ch] = acc;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int v = threadIdx.x;
        double acc = 0.0;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) acc = (MAXMASK >> v & 1u) ? fmax(acc, part[v][ch]) : acc + part[v][ch];
        tot[v] = acc;
    }
    __syncthreads();
}
