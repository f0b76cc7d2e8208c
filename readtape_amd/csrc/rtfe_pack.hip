// rtfe_pack.hip — the event arena of a scan, packed on the device before it crosses PCIe (rtfe_pack_events, include/rt_frontend.h).
//
// rtfe_scan lays the arena out for the worst case: every (burst, parameter set, track) list has event_cap records of room, a fixed share of
// the burst's rows (C2: 38 MB of arena per 2^21 rows hold 6.7 MB of events).  The host replay reads lists, not the arena: what it needs is the
// same addressing rule - events[event_base + (p * ntrks + t) * event_cap + i] - over a smaller buffer.  Two kernels behind the scan, on its stream:
//   k_pack_plan   one workgroup: per burst the longest of its lists (cap2), the bursts' packed bases by a prefix sum, the total
//   k_pack_copy   a workgroup per list, 16 bytes a lane: the list's records to base + list * cap2
// The plan goes to the host with the burst table (16 bytes a burst); the device's burst table is left alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frontend.h"

namespace rtfe {

__global__ void __launch_bounds__(1024) k_pack_plan(const rtfe_burst *__restrict__ bursts, const int32_t *__restrict__ nbursts, long long max_bursts,
                                                    const uint32_t *__restrict__ counts, int lists, rtfe_pack_entry *__restrict__ plan) {
   __shared__ unsigned long long s_v[1024];
   __shared__ unsigned long long s_carry;
   const int tid = threadIdx.x;
   long long nb = *nbursts;
   if (nb > max_bursts) nb = max_bursts;
   if (nb < 0) nb = 0;
   if (tid == 0) s_carry = 0;
   __syncthreads();
   for (long long b0 = 0; b0 < nb; b0 += 1024) {
      const long long b = b0 + tid;
      uint32_t cap2 = 0;
      if (b < nb) {
         const uint32_t *c = counts + (size_t)b * lists;
         for (int l = 0; l < lists; ++l) cap2 = c[l] > cap2 ? c[l] : cap2;
         if (cap2 < 1) cap2 = 1;
         if (cap2 > bursts[b].event_cap) cap2 = bursts[b].event_cap; }        // (a list that overflowed its region: RTFE_F_EVENT_OVERFLOW - the count says what there would have been)
      const unsigned long long n = (unsigned long long)cap2 * (unsigned long long)lists;
      s_v[tid] = n;                                                          // inclusive prefix sum over the workgroup (one workgroup, a few rounds per scan: nothing to optimise)
      __syncthreads();
      for (int s = 1; s < 1024; s <<= 1) {
         const unsigned long long y = tid >= s ? s_v[tid - s] : 0;
         __syncthreads();
         s_v[tid] += y;
         __syncthreads(); }
      const unsigned long long before = s_carry;
      if (b < nb) { rtfe_pack_entry e; e.event_base = before + s_v[tid] - n; e.event_cap = cap2; e.reserved = 0; plan[b] = e; }
      __syncthreads();
      if (tid == 1023) s_carry = before + s_v[1023];
      __syncthreads(); }
   if (tid == 0) { rtfe_pack_entry e; e.event_base = s_carry; e.event_cap = 0; e.reserved = (uint32_t)nb; plan[nb] = e; } }

__global__ void __launch_bounds__(256) k_pack_copy(const rtfe_burst *__restrict__ bursts, const int32_t *__restrict__ nbursts, long long max_bursts,
                                                   const uint32_t *__restrict__ counts, int lists, const rtfe_pack_entry *__restrict__ plan,
                                                   const uint4 *__restrict__ events, uint4 *__restrict__ out, unsigned long long out_cap) {
   long long nb = *nbursts;
   if (nb > max_bursts) nb = max_bursts;
   if (nb <= 0 || plan[nb].event_base > out_cap) return;                        // (does not fit: the host sees the total and fetches the arena as it is)
   const long long npairs = nb * lists;
   for (long long pr = blockIdx.x; pr < npairs; pr += gridDim.x) {
      const long long b = pr / lists;
      const int l = (int)(pr - b * lists);
      const rtfe_pack_entry e = plan[b];
      uint32_t n = counts[pr];
      if (n > e.event_cap) n = e.event_cap;
      const uint4 *src = events + bursts[b].event_base + (unsigned long long)l * bursts[b].event_cap;
      uint4 *dst = out + e.event_base + (unsigned long long)l * e.event_cap;
      for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i]; } }

// The end of the data (src/readtape.c:1410: the reader stops at the first row whose head-0 sample is 0x8000), looked for where the rows already
// are: a strided pass over a window on the host costs as much as reading it.  first[0] = the smallest such row, INT64_MAX if there is none.
__global__ void k_end_mark_init(long long *first) { *first = 0x7fffffffffffffffll; }
__global__ void __launch_bounds__(256) k_end_mark(const int16_t *__restrict__ rows, long long nrows, int ntrks, long long *__restrict__ first) {
   for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += (long long)gridDim.x * blockDim.x)
      if (rows[r * ntrks] == (int16_t)0x8000) atomicMin(reinterpret_cast<unsigned long long *>(first), (unsigned long long)r); }

// -subsample on a raw window (rtfe_decimate_rows, include/rt_frontend.h): out row j = in row first + j * step, and in the same pass k_end_mark's answer over
// EVERY raw row (the reader looks at the marker of the rows it skips too, src/readtape.c:1407-1413).
//
// Rows are 2 * ntrks = 2 .. 38 bytes (nine tracks: 18), so neither the source rows nor the output rows sit on 16-byte boundaries, and a lane that copied its
// own row sample by sample would touch every 64-byte segment many times.  A workgroup is one wave and takes dec_span_rows(ntrks) consecutive raw rows - a
// multiple of 8, so its span starts on a 16-byte boundary of the window - into LDS with 16-byte loads (the last, partial vector of the WINDOW sample by sample:
// no byte behind the last source row is read).  From LDS the lanes
//   - look at head 0 of every row of the span: one minimum over the wave, one atomicMin per workgroup, and none at all where there is no marker;
//   - assemble the workgroup's piece of the output - the kept rows whose source row lies in its span, a contiguous byte range [b_lo, b_hi) of d_out - a 16-byte
//     vector a lane (eight samples, each fetched from where its source row lies in LDS) and store the whole vectors with one 16-byte store; the at most two
//     vectors a workgroup shares with its neighbours (or, at the window's end, with whatever lies behind the output) are written sample by sample, its own
//     samples only.
// Every byte of the window is read once whatever the step; there is no second path for large steps (rows are at most 38 bytes: every 64-byte line holds a
// head-0 sample that the marker search needs).
constexpr int kDecWave = 64;                // a workgroup: one wave
constexpr int kDecLds = 16384;              // bytes of the raw window a workgroup stages: ten workgroups share a CU's 160 KB
inline int dec_span_rows(int ntrks) { return (kDecLds / (2 * ntrks)) & ~7; }      // 904 rows of nine tracks, 424 of nineteen

__global__ void __launch_bounds__(kDecWave) k_decimate(const int16_t *__restrict__ in, long long nrows_in, int ntrks, long long first, long long step, int span,
                                                       int16_t *__restrict__ out, long long *__restrict__ first_mark) {
   __shared__ uint4 s_rows[kDecLds / 16];
   const uint16_t *s16 = reinterpret_cast<const uint16_t *>(s_rows);
   const int lane = threadIdx.x;
   const uint32_t rb = 2u * (uint32_t)ntrks;
   const long long r0 = (long long)blockIdx.x * span;
   const uint32_t nr = (uint32_t)(nrows_in - r0 < span ? nrows_in - r0 : span);      // (the grid is sized so that every workgroup has a row)
   const uint32_t nbytes = nr * rb;
   const unsigned char *src = reinterpret_cast<const unsigned char *>(in) + (size_t)r0 * rb;      // 16-byte aligned: r0 * rb is a multiple of 8 * 2
   const uint32_t nfull = nbytes >> 4;
   for (uint32_t v = lane; v < nfull; v += kDecWave) s_rows[v] = reinterpret_cast<const uint4 *>(src)[v];
   for (uint32_t b = (nfull << 4) + 2u * lane; b < nbytes; b += 2u * kDecWave)                    // (at most seven samples, in the window's last workgroup only)
      reinterpret_cast<uint16_t *>(s_rows)[b >> 1] = *reinterpret_cast<const uint16_t *>(src + b);
   __syncthreads();

   // the end marker: the smallest row of the span whose head-0 sample is 0x8000
   int hit = 0x7fffffff;
   for (uint32_t r = lane; r < nr; r += kDecWave)
      if (s16[(r * rb) >> 1] == 0x8000u && (int)r < hit) hit = (int)r;
   for (int m = 1; m < kDecWave; m <<= 1) { const int o = __shfl(hit, lane ^ m); hit = o < hit ? o : hit; }
   if (lane == 0 && hit != 0x7fffffff) atomicMin(reinterpret_cast<unsigned long long *>(first_mark), (unsigned long long)(r0 + hit));

   // the kept rows whose source row lies in [r0, r0 + nr): j_lo .. j_hi - 1
   const long long r1 = r0 + nr;
   const long long j_lo = r0 <= first ? 0 : (r0 - first + step - 1) / step;
   const long long j_hi = r1 <= first ? 0 : (r1 - first + step - 1) / step;
   if (j_hi <= j_lo) return;
   const uint32_t off0 = (uint32_t)(first + j_lo * step - r0);       // where kept row j_lo lies in the span (rows): below nr
   const uint32_t stp = step < (long long)span ? (uint32_t)step : (uint32_t)span;      // (a step of a span or more: j_lo is the workgroup's only kept row, and stp multiplies 0)
   const unsigned long long b_lo = (unsigned long long)j_lo * rb, b_hi = (unsigned long long)j_hi * rb;
   unsigned char *dst = reinterpret_cast<unsigned char *>(out);
   const uint32_t hop = (stp - 1) * (rb >> 1);                         // samples between the end of a kept row and the start of the next one, in LDS
   for (unsigned long long p = (b_lo & ~15ull) + 16ull * lane; p < b_hi; p += 16ull * kDecWave) {
      const unsigned long long q0 = p > b_lo ? p : b_lo, q1 = p + 16 < b_hi ? p + 16 : b_hi;      // the vector's bytes that are this workgroup's
      const uint32_t q = (uint32_t)(q0 - b_lo);                        // ... counted from kept row j_lo: below nr * rb
      const uint32_t j = q / rb;
      uint32_t c = q - j * rb;                                         // kept row j_lo + j, byte c of it
      uint32_t i = ((off0 + j * stp) * rb + c) >> 1;                   // ... which is sample i of the span
      if (q1 - q0 == 16) {
         uint32_t s[8];
#pragma unroll
         for (int k = 0; k < 8; ++k) {
            s[k] = s16[i++];
            c += 2;
            if (c == rb) { c = 0; i += hop; } }
         *reinterpret_cast<uint4 *>(dst + p) = make_uint4(s[0] | s[1] << 16, s[2] | s[3] << 16, s[4] | s[5] << 16, s[6] | s[7] << 16); }
      else                                                             // shared with a neighbour, or the output's last vector: the own samples, one by one
         for (unsigned long long b = q0; b < q1; b += 2) {
            *reinterpret_cast<uint16_t *>(dst + b) = s16[i++];
            c += 2;
            if (c == rb) { c = 0; i += hop; } } } }

}  // namespace rtfe
