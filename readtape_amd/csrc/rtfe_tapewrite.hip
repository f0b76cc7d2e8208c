// rtfe_tapewrite.hip — a slot stream and a block table -> the int16 rows of the tape they describe (rtfe_tape_render, include/rt_frontend.h): the decoders'
// other direction.  The bytes are the host renderer's (csrc/host/rt_tapewrite.c), which are readtape_amd/synth.py's: the expressions that decide them are
// host/rt_tapewrite_model.h, compiled into both.  What differs is the walk: the host adds pulse after pulse into an array of doubles; here a lane owns a
// SAMPLE and sums the pulses that reach it, in ascending slot order from 0.0 - the order the host's additions arrive in at that sample.
//
// Layout.  A workgroup (256 lanes) takes a span of kTwSpanRows rows on the tape's own grid, clipped to the window.  It finds the first block that ends behind
//   the span's first row by bisection of the block table, and walks the blocks up to the span's end: the rows in front of a block are gap - a lane a sample,
//   one hash and the quantiser, no slot is fetched (a span without a block is only this) -; for the rows the span shares with a block the slots that can reach
//   them (the rows' cells, the reach K, the largest skew and the generator's bounded jitter: `reach` rows either side, computed by the host) are staged in LDS
//   once, and a lane walks the slots that can reach ITS row, tests its track's bit and the model's |r - rint(c)| <= K, and adds.  Only a block's own rows take
//   its pulses, so a sample has one block at the most.  The int16 samples go to LDS at the place their bytes have counted from the 16-byte boundary in front
//   of the span's first byte in d_rows; the workgroup then stores whole aligned 16-byte vectors and, sample by sample, the partial ones at its two ends (a row
//   of nine tracks is 18 bytes, and the window starts anywhere on the grid).  Nothing is written outside d_rows[0 .. nrows * ntrks).
// Cost.  Two double divisions a pulse and one a sample (the quantiser), written as divisions: they are the model's roundings, and no restatement of them that is
//   exact for every operand is known to this file (DESIGN.md 4i has the measured rate and what bounds it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frontend.h"
#define RT_TW_FN __host__ __device__ static __forceinline__
#include "host/rt_tapewrite_model.h"

namespace rtfe {

constexpr int kTwThreads = 256;
constexpr int kTwSpanRows = 256;                    // rows a workgroup takes: 256 * ntrks * 2 bytes, a multiple of 16 for every track count
constexpr int kTwSlotCap = RTFE_TAPE_MAX_SLOTS;     // slots staged for one block's share of a span (16 KB)
constexpr int kTwOutVecs = (kTwSpanRows * RTFE_MAXTRKS * 2 + 16 + 15) / 16;

struct TapeArgs {
   const rtfe_tape_slot *slots;
   const rtfe_tape_block *blocks; long long nblocks;
   long long first_row, nrows, span0;               // the window; the first span of the tape's grid that it touches
   int16_t *rows;
   long long reach;                                 // rows either side of a row within which a slot's nominal place can lie and still reach it
   double slots_per_row, lead_rows;                 // 1 / (spb * pitch); (8 + 0.5) * spb
   rtfe_tape_params p;
};

// the slots that can reach row r of a block: a superset, [lo, hi] before clamping (the truncation and the +-2 swallow every rounding of these two lines)
__device__ __forceinline__ long long tw_slot_lo(const TapeArgs &a, long long r) { return (long long)(((double)(r - a.reach) - a.lead_rows) * a.slots_per_row) - 2; }
__device__ __forceinline__ long long tw_slot_hi(const TapeArgs &a, long long r) { return (long long)(((double)(r + a.reach) - a.lead_rows) * a.slots_per_row) + 2; }

__global__ void __launch_bounds__(kTwThreads) k_tape_render(const TapeArgs a) {
   __shared__ uint4 s_out4[kTwOutVecs];
   __shared__ rtfe_tape_slot s_slot[kTwSlotCap];
   __shared__ double s_amp[RTFE_MAXTRKS], s_skew[RTFE_MAXTRKS];
   __shared__ unsigned long long s_nkey[RTFE_MAXTRKS], s_jkey[RTFE_MAXTRKS];
   int16_t *s_out = reinterpret_cast<int16_t *>(s_out4);
   const unsigned tid = threadIdx.x, nt = (unsigned)a.p.ntrks;
   if (tid < nt) { s_amp[tid] = a.p.amp[tid]; s_skew[tid] = a.p.skew[tid]; s_nkey[tid] = a.p.nkey[tid]; s_jkey[tid] = a.p.jkey[tid]; }
   const long long w1 = a.first_row + a.nrows, g0 = (a.span0 + (long long)blockIdx.x) * kTwSpanRows;
   const long long lo = g0 > a.first_row ? g0 : a.first_row, hi = g0 + kTwSpanRows < w1 ? g0 + kTwSpanRows : w1;      // (the grid has no span without a row)
   const unsigned long long b_lo = (unsigned long long)(lo - a.first_row) * nt * 2u, b_hi = (unsigned long long)(hi - a.first_row) * nt * 2u, a0 = b_lo & ~15ull;
   const unsigned shift = (unsigned)((b_lo - a0) >> 1);                         // where row lo's first sample lies in s_out
   long long bl = 0, bh = a.nblocks;                                            // the first block that ends behind lo
   while (bl < bh) {
      const long long mid = bl + ((bh - bl) >> 1);
      if (a.blocks[mid].first_row + a.blocks[mid].rows <= lo) bl = mid + 1; else bh = mid; }
   __syncthreads();
   const double noise_mv = a.p.noise_mv, maxvolts = a.p.maxvolts;

   auto gap = [&](long long x0, long long x1) {                                 // rows [x0, x1) of the tape belong to no block
      const unsigned n = (unsigned)(x1 - x0) * nt;
      for (unsigned e = tid; e < n; e += kTwThreads) {
         const unsigned dr = e / nt, t = e - dr * nt;
         const double v = 0.0 + rt_tw_noise(noise_mv, s_nkey[t], x0 + dr);
         s_out[shift + (unsigned)(x0 - lo) * nt + e] = rt_tw_quantise(v, maxvolts); } };

   long long cur = lo;
   for (long long b = bl; b < a.nblocks; ++b) {
      const rtfe_tape_block B = a.blocks[b];
      if (B.first_row >= hi) break;
      const long long r0 = B.first_row > lo ? B.first_row : lo, r1 = B.first_row + B.rows < hi ? B.first_row + B.rows : hi;
      if (r0 > cur) gap(cur, r0);
      const long long q0 = r0 - B.first_row, q1 = r1 - B.first_row;              // the block's rows [q0, q1), counted from its first
      long long s_first = tw_slot_lo(a, q0), s_last = tw_slot_hi(a, q1 - 1);
      if (s_first < 0) s_first = 0;
      if (s_last > B.nslots - 1) s_last = B.nslots - 1;
      long long count = s_last - s_first + 1;
      if (count > kTwSlotCap) count = kTwSlotCap;                               // (the host refuses what would come here: -60)
      for (long long i = tid; i < count; i += kTwThreads) s_slot[i] = a.slots[B.first_slot + s_first + i];
      __syncthreads();
      const unsigned n = (unsigned)(q1 - q0) * nt;
      for (unsigned e = tid; e < n; e += kTwThreads) {
         const unsigned dr = e / nt, t = e - dr * nt;
         const long long r = q0 + dr;
         long long sl = tw_slot_lo(a, r), sh = tw_slot_hi(a, r);
         if (sl < s_first) sl = s_first;
         if (sh > s_first + count - 1) sh = s_first + count - 1;
         const double amp = s_amp[t], skew = s_skew[t];
         const unsigned long long jkey = s_jkey[t];
         double v = 0.0;
         for (long long s = sl; s <= sh; ++s) {
            const rtfe_tape_slot sl8 = s_slot[s - s_first];
            if (!((sl8.flux >> t) & 1u)) continue;
            const double c = rt_tw_centre(a.p.spb, a.p.pitch_shift, skew, a.p.jitter, jkey, s, B.first_slot + s);
            const long long dlt = r - (long long)rint(c);
            if (dlt < -(long long)a.p.K || dlt > (long long)a.p.K) continue;
            v += rt_tw_pulse(((sl8.neg >> t) & 1u) ? -amp : amp, r, c, a.p.w, a.p.edge); }
         v = v + rt_tw_noise(noise_mv, s_nkey[t], r0 + dr);
         s_out[shift + (unsigned)(r0 - lo) * nt + e] = rt_tw_quantise(v, maxvolts); }
      __syncthreads();                                                          // (the next block's slots overwrite these)
      cur = r1; }
   if (hi > cur) gap(cur, hi);
   __syncthreads();
   unsigned char *out = reinterpret_cast<unsigned char *>(a.rows);
   for (unsigned long long p = a0 + 16ull * tid; p < b_hi; p += 16ull * kTwThreads) {
      if (p >= b_lo && p + 16 <= b_hi) *reinterpret_cast<uint4 *>(out + p) = s_out4[(p - a0) >> 4];
      else {                                                                    // the vector holds a neighbouring span's samples too, or the window ends inside it
         const unsigned long long e0 = p > b_lo ? p : b_lo, e1 = p + 16 < b_hi ? p + 16 : b_hi;
         for (unsigned long long q = e0; q < e1; q += 2) *reinterpret_cast<int16_t *>(out + q) = s_out[(q - a0) >> 1]; } } }

}  // namespace rtfe
