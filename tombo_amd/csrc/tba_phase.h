// tba_phase.h -- the profiling builds of the kernels, all of it: the switches, the two clocks the kernels
// carry, and what every build leaves in ReadState.dbg[0..7] (read back with TBA_GET_DEBUG_COUNTERS).
// Nothing else in csrc/ tests a profiling switch with the preprocessor: the kernels hold a clock whose
// methods are empty, and which has no members, unless its build is the one being compiled.
//
//   -DTBA_PHASE_DEBUG=<id>     dbg[] of the read (cycles = shader clock, s_memtime)
//    1 k_peaks          stamps: 0 tiles, 1 global rounds, 2 range of the taken scores, 3 k-th score, 4 = 5 picks; 7
//    2 k_normalize      stamps: 0 sample range, 1 median, 2 MAD, 3 third median / limits, 4 norm written; 7
//    3 k_theil_sen      stamps: 0 points, 1 window sample, 6 tolerance, 2 pass over the pairs, 3 fast select,
//                       4 generic select, 5 intercept; 7
//    4 k_peaks tiles    wave 0, summed over its tiles: 0 masks, 1 rounds, 2 emission; 3 rounds, 4 tiles (counts)
//    5 k_dp row parts   lane 0 of k_dp's main pass, summed over the rows: 0 z-scores, 1 candidates, 2 first scan
//                       + sweeps, 3 cells / flags / stores / ring upkeep, 4 arg-max, 5 band placement; 6 rows;
//                       7 where the wavefront ran: HW_ID (wave slot [3:0], SIMD [5:4], CU [11:8], SH [12],
//                       SE [15:13]) | XCC_ID << 32
//    7 k_detect roles   of the workgroup's FIRST read, summed over the steps: 0 scan (wave 0), 1 loader (wave 1),
//                       2 greedy (wave 2) = 3 masks + 4 rounds + 5 emission + 6 tail; 7 steps
//    8 k_pick           stamps: 0 select + counts, 1 offsets, 2 compaction; 7
//    9 k_detect_tt      cycles inside a step's work: 0 greedy wavefront, 1 scorer wave 1, 4 scorer wave 7;
//                       2 the whole loop, 3 tiles
//   11 k_stall_metric   thread 0 of every workgroup, added up per read: 0 sums into LDS, 1 moving averages,
//                       2 metric; 3 chunks, 4 workgroups
//   12 k_main_tb_par    counts added up per read: 0 lanes that extended, 1 merged at once, 2 merged later, 3 rows
//                       overwritten in phase B, 4 chunks, 5 sum of (chunk top - row merged at), 6 lanes whose
//                       phase A died, 7 sum of phase-A start states
//   13 k_skip_dp        the read's wavefront: 0 whole kernel, 1 its window loops, 2 column phase, 3 flat phase;
//                       6 windows
//   ("stamps": cycles since the kernel's start, thread 0; 7 = the same interval on the constant 100 MHz
//   counter, which gives the shader clock of the run)
//   -DTBA_SWEEP_STATS          k_dp main pass: 0 rows, 1 stay-chain sweeps
//   -DTBA_SKIP_STATS           k_skip_dp_wave, added up over the read's windows: 0 windows, 1 cycles, 2 cells,
//                              3 .. 7 parts of a base (wait, z-scores, diagonal sources, stay chain, flags)
//   -DTBA_SKIP_CLASS_STATS     k_skip_dp_wave, per class c = 0 .. 2: c windows, 3 + c cycles
// Every one of these writes dbg[0], so a build takes ONE switch: no combination is allowed.
#pragma once

#ifdef TBA_PHASE_DEBUG
constexpr int TBA_PHASE_ID = TBA_PHASE_DEBUG;
#else
constexpr int TBA_PHASE_ID = 0;
#endif
#ifdef TBA_SWEEP_STATS
constexpr bool TBA_SWEEP_STATS_ON = true;
#else
constexpr bool TBA_SWEEP_STATS_ON = false;
#endif
#ifdef TBA_SKIP_STATS
constexpr bool TBA_SKIP_STATS_ON = true;
#else
constexpr bool TBA_SKIP_STATS_ON = false;
#endif
#ifdef TBA_SKIP_CLASS_STATS
constexpr bool TBA_SKIP_CLASS_STATS_ON = true;
#else
constexpr bool TBA_SKIP_CLASS_STATS_ON = false;
#endif
enum { PH_PEAKS = 1, PH_NORMALIZE = 2, PH_THEIL_SEN = 3, PH_PEAKS_TILES = 4, PH_DP_ROW = 5, PH_DETECT = 7,
       PH_PICK = 8, PH_DETECT_TT = 9, PH_STALL_METRIC = 11, PH_TB_PAR = 12, PH_SKIP_DP = 13 };
constexpr bool phase_on(int id) { return TBA_PHASE_ID == id; }
static_assert(TBA_PHASE_ID == 0 || (TBA_PHASE_ID >= 1 && TBA_PHASE_ID <= 13 && TBA_PHASE_ID != 6 && TBA_PHASE_ID != 10),
              "TBA_PHASE_DEBUG: no such kernel id (see the table in tba_phase.h)");
static_assert((TBA_PHASE_ID != 0) + TBA_SWEEP_STATS_ON + TBA_SKIP_STATS_ON + TBA_SKIP_CLASS_STATS_ON <= 1,
              "TBA_PHASE_DEBUG, TBA_SWEEP_STATS, TBA_SKIP_STATS and TBA_SKIP_CLASS_STATS write the same "
              "ReadState.dbg slots: one profiling switch per build");

__device__ __forceinline__ i64 phase_cycles() { return (i64)__builtin_readcyclecounter(); }
__device__ __forceinline__ i64 phase_hw_id() // HW_ID | XCC_ID << 32 of the wavefront (scalar registers only)
{
    u32 hw_id, xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    return (i64)hw_id | ((i64)(xcc_id & 15) << 32);
}

// Stamp clock: thread 0 stores the cycles since construction into dbg[i], and at the end the 100 MHz interval into dbg[7].
template <bool ON> struct StampClock {
    __device__ __forceinline__ explicit StampClock(i64 *) {}
    __device__ __forceinline__ void stamp(int) const {}
    __device__ __forceinline__ void end() const {}
};
template <> struct StampClock<true> {
    i64 *dbg, t0, w0;
    __device__ __forceinline__ explicit StampClock(i64 *d) : dbg(d), t0(phase_cycles()), w0((i64)__builtin_amdgcn_s_memrealtime()) {}
    __device__ __forceinline__ void stamp(int i) const { if (threadIdx.x == 0) dbg[i] = phase_cycles() - t0; }
    __device__ __forceinline__ void end() const { if (threadIdx.x == 0) dbg[7] = (i64)__builtin_amdgcn_s_memrealtime() - w0; }
};

// Lap clock: N accumulators in registers.  lap(i) adds the cycles since the previous lap (or mark) to accumulator i,
// count(i, v) adds v; flush* write accumulators [lo, hi) to the same slots of dbg.  WHO writes is the caller's `if`
// (lane 0, thread 0, every lane), HOW is the method: store, add, or atomicAdd where workgroups share a read.
template <int N, bool ON> struct LapClock {
    __device__ __forceinline__ void mark() {}
    __device__ __forceinline__ void lap(int) {}
    __device__ __forceinline__ void count(int, i64 = 1) {}
    __device__ __forceinline__ i64 get(int) const { return 0; }
    __device__ __forceinline__ i64 since_start() const { return 0; }
    __device__ __forceinline__ void flush(i64 *, int, int) const {}
    __device__ __forceinline__ void flush_add(i64 *, int, int) const {}
    __device__ __forceinline__ void flush_atomic(i64 *, int, int) const {}
};
template <int N> struct LapClock<N, true> {
    i64 acc[N] = {}, t0 = phase_cycles(), t = t0;
    __device__ __forceinline__ void mark() { t = phase_cycles(); }
    __device__ __forceinline__ void lap(int i) { const i64 n = phase_cycles(); acc[i] += n - t; t = n; }
    __device__ __forceinline__ void count(int i, i64 v = 1) { acc[i] += v; }
    __device__ __forceinline__ i64 get(int i) const { return acc[i]; }
    __device__ __forceinline__ i64 since_start() const { return phase_cycles() - t0; }
    __device__ __forceinline__ void flush(i64 *dbg, int lo, int hi) const
    {
#pragma unroll
        for (int i = 0; i < N; i++) if (i >= lo && i < hi) dbg[i] = acc[i];
    }
    __device__ __forceinline__ void flush_add(i64 *dbg, int lo, int hi) const
    {
#pragma unroll
        for (int i = 0; i < N; i++) if (i >= lo && i < hi) dbg[i] += acc[i];
    }
    __device__ __forceinline__ void flush_atomic(i64 *dbg, int lo, int hi) const
    {
#pragma unroll
        for (int i = 0; i < N; i++)
            if (i >= lo && i < hi) atomicAdd((unsigned long long *)&dbg[i], (unsigned long long)acc[i]);
    }
};
