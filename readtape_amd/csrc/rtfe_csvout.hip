// rtfe_csvout.hip — int16 rows in device memory -> the text of the converter's -read (rtfe_csv_format, include/rt_frontend.h): rtfe_csv.hip's mirror image.
//
// The text is the host writer's (csrc/host/rt_csvout.c, which restates src/csvtbin.c:570-595), byte for byte: a line is "%12.8f, " of (double)t_ns / 1e9,
// then "%9.5f, " of every column's float32 value, then '\n'.  printf is not here; both fields are made in integer arithmetic that is exact:
//
// The voltage field.  f is computed as the reference computes it (float32, the divide and the multiply rounded apart: -ffp-contract=off; the stagger summed in
//   float32).  A finite float is exactly (-1)^s * m * 2^e with m < 2^24, so the number printf rounds is m * 10^5 * 2^e, and N = the nearest integer to it, ties to
//   even (glibc rounds the exact binary value in the current rounding mode), is what the five decimals and the digits in front of them spell.  m * 10^5 < 2^41
//   fits 64 bits; the domain the API admits (|f| < 2^21) has e < 0, so N is a right shift of that product with the remainder compared against one half - no
//   rounding happens before the one that counts.  A shift of 64 or more leaves nothing: N = 0.  The '-' is the sign BIT (printf prints -0.00000 for -0.0f and for
//   a negative value that rounds to zero).
//
// The time field.  q = (double)t / 1e9 is one IEEE division: t < 2^49 converts exactly, and a double division on this target is the correctly rounded one
//   (v_div_scale / v_rcp / the FMA refinement / v_div_fmas / v_div_fixup: the compiler has no approximate form for f64 unless fast-math asks for it, which this
//   build forbids) - the same q the host's divsd gives.  printf then rounds the exact value of q to 8 decimals.  Let t = 10 k + d.
//     d != 5:  q = (t / 1e9)(1 + eps), |eps| <= 2^-53, so |q * 1e8 - t / 10| <= (t / 10) 2^-53 < 2^49 / 10 / 2^53 < 0.007, while t / 10 = k + d / 10 lies at
//              least 0.1 from k + 1/2: q * 1e8 rounds where t / 10 does, to k + (d > 5).
//     d == 5:  t / 10 = k + 1/2 exactly, so q * 1e8 is above, below or on the tie as q is above, below or equal to t / 1e9, that is as q * 1e9 - t is positive,
//              negative or zero.  fma(q, 1e9, -t) computes that difference with ONE rounding, which cannot change the sign of a non-zero value nor make zero
//              of one (it is a multiple of 2^-76 and far from the subnormals).  Zero is a true tie (t = 1953125 ns = 2^-9 s): half to even, k + (k & 1).
//   k < 2^49 / 10; its eight low decimal digits are the fraction.
//
// Layout.  A workgroup is one wave and formats `lines` consecutive rows, a lane a row, into LDS, at the place each byte has in the window's text counted from
//   the 16-byte boundary in front of the workgroup's first line; the wave then copies whole aligned 16-byte vectors out (a line is 113 bytes: a lane storing
//   its own line byte by byte would touch every 64-byte segment 64 times), and the at most two partial vectors at its ends - shared with the neighbouring
//   workgroups - byte by byte.  Where a line starts:
//     uniform   the host has proved every line of the window 14 + 11 ntrks + 1 bytes long (every time below 1000 s, every |f| below 99): a multiplication;
//     general   k_csvout_len: the workgroups' byte counts (the same digit counts, nothing stored); k_csvout_scan: their exclusive prefix sum, the window's
//               total and RTFE_CSV_TEXT_FULL; the format kernel adds the prefix sum of its own lanes' lengths.
//   Nothing is written at or behind text_cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frontend.h"

namespace rtfe {

constexpr int kCoWave = 64;                 // a workgroup: one wave, a lane a line
constexpr int kCoLds = 16384;               // bytes of text a workgroup stages: 64 uniform lines of nineteen tracks (224 bytes) and 64 worst-case lines of nine (162) fit; ten workgroups share a CU's 160 KB
constexpr int kCoTimeMax = 17;              // "562949.95342131, "  (t < 2^49 ns)
constexpr int kCoVoltMax = 16;              // "-2097152.00000, "   (|f| < 2^21)
constexpr int kCoScanThreads = 1024;

inline int co_max_line(int ntrks) { return kCoTimeMax + kCoVoltMax * ntrks + 1; }
inline int co_uniform_line(int ntrks) { return 14 + 11 * ntrks + 1; }
inline int co_lines_per_wg(int line_bytes) { const int n = (kCoLds - 16) / line_bytes; return n < kCoWave ? n : kCoWave; }

struct CsvFormatArgs {
   const int16_t *rows;                     // row 0 of the tape
   long long first_row, nrows;              // the window
   int ntrks, invert;
   float maxvolts, stagger;
   unsigned long long tstart; uint32_t tdelta;
   unsigned long long perm_lo, perm_hi;     // the column of the rows that field k prints, 5 bits each: fields 0 .. 11 | 12 .. 18
   int lines;                               // rows a workgroup formats (co_lines_per_wg)
   uint32_t uniform_len;                    // the uniform path: every line's length
   const unsigned long long *base;          // the general path: where each workgroup's first line starts
   unsigned char *text; unsigned long long text_cap;
};

__device__ __forceinline__ int co_ndigits(uint32_t v) {
   return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10; }

// v as nd decimal digits (leading zeros) at o[p ..]; kWrite = false only counts.  -> the position behind them
template <bool kWrite> __device__ __forceinline__ int co_digits(unsigned char *o, int p, uint32_t v, int nd) {
   if (kWrite) for (int i = nd - 1; i >= 0; --i) { const uint32_t q = v / 10u; o[p + i] = (unsigned char)('0' + (v - q * 10u)); v = q; }
   return p + nd; }
template <bool kWrite> __device__ __forceinline__ int co_fill(unsigned char *o, int p, int n, unsigned char c) {
   if (kWrite) for (int i = 0; i < n; ++i) o[p + i] = c;
   return p + (n > 0 ? n : 0); }

// "%12.8f, " of (double)t / 1e9 (the proof is at the top of the file)
template <bool kWrite> __device__ __forceinline__ int co_time(unsigned char *o, int p, unsigned long long t) {
   unsigned long long k = t / 10u;
   const unsigned d = (unsigned)(t - k * 10u);
   if (d > 5) ++k;
   else if (d == 5) {
      const double q = (double)t / 1e9;
      const double r = fma(q, 1e9, -(double)t);
      if (r > 0 || (r == 0 && (k & 1))) ++k; }
   const unsigned long long sec = k / 100000000ull;
   const uint32_t s = (uint32_t)sec, frac = (uint32_t)(k - sec * 100000000ull);
   const int nd = co_ndigits(s);
   p = co_fill<kWrite>(o, p, 3 - nd, ' ');
   p = co_digits<kWrite>(o, p, s, nd);
   if (kWrite) o[p] = '.';
   p = co_digits<kWrite>(o, p + 1, frac, 8);
   if (kWrite) { o[p] = ','; o[p + 1] = ' '; }
   return p + 2; }

// "%9.5f, " of f
template <bool kWrite> __device__ __forceinline__ int co_volt(unsigned char *o, int p, float f) {
   const uint32_t b = __float_as_uint(f);
   const int neg = (int)(b >> 31), E = (int)((b >> 23) & 255u);
   uint32_t m = b & 0x7FFFFFu;
   int s = 149;                                                                 // |f| = m * 2^-s
   if (E) { m |= 1u << 23; s = 150 - E; }
   const unsigned long long P = (unsigned long long)m * 100000ull;
   unsigned long long N = P;                                                    // (s <= 0 is |f| >= 2^23: the API admits no such value)
   if (s >= 64) N = 0;
   else if (s > 0) {
      N = P >> s;
      const unsigned long long rem = P & ((1ull << s) - 1), half = 1ull << (s - 1);
      if (rem > half || (rem == half && (N & 1))) ++N; }
   const unsigned long long whole = N / 100000ull;
   const uint32_t w = (uint32_t)whole, frac = (uint32_t)(N - whole * 100000ull);
   const int nd = co_ndigits(w);
   p = co_fill<kWrite>(o, p, 9 - (neg + nd + 6), ' ');
   if (neg) { if (kWrite) o[p] = '-'; ++p; }
   p = co_digits<kWrite>(o, p, w, nd);
   if (kWrite) o[p] = '.';
   p = co_digits<kWrite>(o, p + 1, frac, 5);
   if (kWrite) { o[p] = ','; o[p + 1] = ' '; }
   return p + 2; }

// the line of row r of the tape at o[0 ..] -> its length
template <bool kWrite> __device__ __forceinline__ int co_line(const CsvFormatArgs &a, long long r, unsigned char *o) {
   int p = co_time<kWrite>(o, 0, a.tstart + (unsigned long long)r * a.tdelta);
   const int16_t *row = a.rows + r * a.ntrks;
   float amount = 0.f;
   for (int k = 0; k < a.ntrks; ++k) {
      const int col = (int)((k < 12 ? a.perm_lo >> (5 * k) : a.perm_hi >> (5 * (k - 12))) & 31u);
      float f = (float)row[col] / 32767 * a.maxvolts;                           // src/csvtbin.c:587-590, operation for operation
      if (a.invert) f = -f;
      f += amount;
      amount += a.stagger;
      p = co_volt<kWrite>(o, p, f); }
   if (kWrite) o[p] = '\n';
   return p + 1; }

// sums[wg] = the bytes of the workgroup's lines; the longest line
__global__ void __launch_bounds__(kCoWave) k_csvout_len(const CsvFormatArgs a, unsigned long long *__restrict__ sums, rtfe_csv_text *__restrict__ out) {
   const int lane = threadIdx.x;
   const long long j = (long long)blockIdx.x * a.lines + lane;
   int len = 0;
   if (lane < a.lines && j < a.nrows) len = co_line<false>(a, a.first_row + j, nullptr);
   const int total = csv_wave_sum(len), longest = csv_wave_max(len);
   if (lane == 0) {
      sums[blockIdx.x] = (unsigned long long)total;
      atomicMax(reinterpret_cast<int *>(&out->longest), longest); } }

// in place: sums[wg] -> the bytes in front of workgroup wg; the window's totals (k_csv_scan's pattern: one workgroup, rounds of 1024 with a carry)
__global__ void __launch_bounds__(kCoScanThreads) k_csvout_scan(uint32_t nwg, unsigned long long *__restrict__ sums, long long nrows, unsigned long long text_cap,
                                                                rtfe_csv_text *__restrict__ out) {
   __shared__ unsigned long long s_v[kCoScanThreads];
   __shared__ unsigned long long s_carry;
   const int tid = threadIdx.x;
   if (tid == 0) s_carry = 0;
   __syncthreads();
   for (uint32_t b0 = 0; b0 < nwg; b0 += kCoScanThreads) {
      const uint32_t b = b0 + tid;
      const unsigned long long v = b < nwg ? sums[b] : 0;
      s_v[tid] = v;
      __syncthreads();
      for (int s = 1; s < kCoScanThreads; s <<= 1) {
         const unsigned long long y = tid >= s ? s_v[tid - s] : 0;
         __syncthreads();
         s_v[tid] += y;
         __syncthreads(); }
      const unsigned long long carry = s_carry;
      if (b < nwg) sums[b] = carry + s_v[tid] - v;
      __syncthreads();
      if (tid == kCoScanThreads - 1) s_carry = carry + s_v[tid];
      __syncthreads(); }
   if (tid == 0) { out->bytes = s_carry; out->rows = nrows; out->flags = s_carry > text_cap ? RTFE_CSV_TEXT_FULL : 0; } }

// the uniform path's totals (the host knows them; they are reported where the general path reports its own)
__global__ void k_csvout_total(rtfe_csv_text *out, unsigned long long bytes, long long nrows, uint32_t longest, unsigned long long text_cap) {
   out->bytes = bytes; out->rows = nrows; out->longest = longest; out->flags = bytes > text_cap ? RTFE_CSV_TEXT_FULL : 0; }

template <bool kUniform> __global__ void __launch_bounds__(kCoWave) k_csvout_format(const CsvFormatArgs a) {
   __shared__ uint4 s_text[kCoLds / 16];
   unsigned char *s = reinterpret_cast<unsigned char *>(s_text);
   const int lane = threadIdx.x;
   const long long j0 = (long long)blockIdx.x * a.lines, j = j0 + lane;
   const bool active = lane < a.lines && j < a.nrows;
   unsigned long long lo, off, e1;                                              // the workgroup's first byte, this lane's line, behind the workgroup's last byte
   if (kUniform) {
      const long long nl = a.nrows - j0 < a.lines ? a.nrows - j0 : a.lines;
      lo = (unsigned long long)j0 * a.uniform_len;
      off = (unsigned long long)j * a.uniform_len;
      e1 = lo + (unsigned long long)nl * a.uniform_len; }
   else {
      const int len = active ? co_line<false>(a, a.first_row + j, nullptr) : 0;
      int incl = len;
      for (int dlt = 1; dlt < kCoWave; dlt <<= 1) { const int y = __shfl_up(incl, dlt); if (lane >= dlt) incl += y; }
      lo = a.base[blockIdx.x];
      off = lo + (unsigned long long)(incl - len);
      e1 = lo + (unsigned long long)__shfl(incl, kCoWave - 1); }
   const unsigned long long a0 = lo & ~15ull;
   if (active) co_line<true>(a, a.first_row + j, s + (off - a0));                // (off - a0) + the line's length <= 15 + lines * the longest possible line <= kCoLds
   __syncthreads();
   const unsigned long long end = e1 < a.text_cap ? e1 : a.text_cap;
   for (unsigned long long p = a0 + 16ull * lane; p < end; p += 16ull * kCoWave) {
      if (p >= lo && p + 16 <= end) *reinterpret_cast<uint4 *>(a.text + p) = s_text[(p - a0) >> 4];
      else {                                                                    // the vector holds a neighbour's bytes too, or the cap cuts it
         const unsigned long long b0 = p > lo ? p : lo, b1 = p + 16 < end ? p + 16 : end;
         for (unsigned long long b = b0; b < b1; ++b) a.text[b] = s[b - a0]; } } }

}  // namespace rtfe
