// rtfe_csv.hip — CSV text in device memory -> the int16 rows a scan takes (rtfe_csv_index / _peak / _parse, include/rt_frontend.h).
//
// The numbers are the host loader's (csrc/host/rt_csv.c, which restates src/csvtbin.c:619-716): the same byte loops, the same float
// recurrences operation for operation (-ffp-contract=off, IEEE division), the same quantiser.  What is new is where they run: a WINDOW of the
// file's bytes (16-byte aligned, readable up to its length rounded up to 16, shorter than 2^32) lies in device memory, and
//   k_csv_count   a workgroup per 4 KB block, 16 bytes a lane: the block's newlines and where its last one ends
//   k_csv_scan    one workgroup: the blocks' offsets into the table of line starts (a prefix sum) and the start of the line each block
//                 opens in (a running maximum); the window's line count, `consumed`, the line behind the last newline of the file
//   k_csv_starts  the blocks again: starts[i] = the offset of line i's first byte; the longest line
//   k_csv_peak    a lane per surveyed line: max |v * scale| (rt_csv_survey's peak)
//   k_csv_parse   a lane per kept line: the line's int16 codes (rt_csv_load's row)
//   k_csv_graph   a lane per kept line: max |v * scale| into the bin its sample number falls in (the converter's -graph) and into the pass's peak (-redo)
// A line ends behind its '\n'; its end bounds the scanners the way the terminating NUL of the host's line buffer does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_frontend.h"

namespace rtfe {

constexpr int kCsvLaneBytes = 16;          // k_csv_count / k_csv_starts: bytes a lane looks at (one uint4 load)
constexpr int kCsvBlockBytes = 4096;       // ... and a workgroup of 256 lanes
constexpr int kCsvWaveLines = 64;          // k_csv_peak / k_csv_parse: a workgroup is one wave, a lane per line
constexpr int kCsvLdsBudget = 8192;        // bytes of text a wave stages into LDS (its 64 lines from the 16-byte boundary in front of the first); a longer span is read
                                           // where it lies.  8 KB: 64 lines of a nine-track export (104 bytes) fit, and nineteen one-wave workgroups share a CU's 160 KB
constexpr int kCsvScanThreads = 1024;

// the 4-bit mask of the bytes of w that are '\n' (bit i: byte i, the lowest address first)
__device__ __forceinline__ uint32_t csv_nl4(uint32_t w) {
   const uint32_t x = w ^ 0x0A0A0A0Au;
   const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // 0x80 in every byte of x that is zero (exact: no carry leaves a byte)
   return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u); }

// the 16-bit newline mask of a lane's chunk; chunks and bytes behind the window's end read as "no newline"
__device__ __forceinline__ uint32_t csv_chunk_mask(const uint4 *__restrict__ text, uint32_t nbytes, uint32_t chunk) {
   const unsigned long long at = (unsigned long long)chunk * kCsvLaneBytes;
   if (at >= nbytes) return 0;
   const uint4 q = text[chunk];
   uint32_t m = csv_nl4(q.x) | (csv_nl4(q.y) << 4) | (csv_nl4(q.z) << 8) | (csv_nl4(q.w) << 12);
   const unsigned long long left = nbytes - at;
   if (left < kCsvLaneBytes) m &= (1u << (unsigned)left) - 1u;
   return m; }

__device__ __forceinline__ int csv_wave_max(int v) {
   const int lane = threadIdx.x & 63;
   for (int m = 1; m < 64; m <<= 1) { const int o = __shfl(v, lane ^ m); v = o > v ? o : v; }
   return v; }
__device__ __forceinline__ int csv_wave_sum(int v) {
   const int lane = threadIdx.x & 63;
   for (int m = 1; m < 64; m <<= 1) v += __shfl(v, lane ^ m);
   return v; }

// cnt[b] = newlines of block b, last[b] = the offset behind its last newline (0: it has none)
__global__ void __launch_bounds__(256) k_csv_count(const uint4 *__restrict__ text, uint32_t nbytes, uint32_t *__restrict__ cnt, uint32_t *__restrict__ last) {
   __shared__ uint32_t s_c[256], s_l[256];
   const int tid = threadIdx.x;
   const uint32_t chunk = blockIdx.x * 256u + tid;
   const uint32_t m = csv_chunk_mask(text, nbytes, chunk);
   s_c[tid] = __popc(m);
   s_l[tid] = m ? chunk * kCsvLaneBytes + (32 - __clz((int)m)) : 0;
   __syncthreads();
   for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) { s_c[tid] += s_c[tid + s]; s_l[tid] = s_l[tid + s] > s_l[tid] ? s_l[tid + s] : s_l[tid]; }
      __syncthreads(); }
   if (tid == 0) { cnt[blockIdx.x] = s_c[0]; last[blockIdx.x] = s_l[0]; } }

// in place: cnt[b] -> newlines in front of block b, last[b] -> where the line that block b opens in starts; then the window's totals
// (the house pattern of k_pack_plan: one workgroup, rounds of 1024 with a carry)
__global__ void __launch_bounds__(kCsvScanThreads) k_csv_scan(uint32_t nblocks, uint32_t nbytes, int is_last, uint32_t *__restrict__ cnt, uint32_t *__restrict__ last,
                                                             uint32_t *__restrict__ starts, long long starts_cap, rtfe_csv_window *__restrict__ out) {
   __shared__ uint32_t s_c[kCsvScanThreads], s_l[kCsvScanThreads];
   __shared__ uint32_t s_carry_c, s_carry_l;
   const int tid = threadIdx.x;
   if (tid == 0) { s_carry_c = 0; s_carry_l = 0; }
   __syncthreads();
   for (uint32_t b0 = 0; b0 < nblocks; b0 += kCsvScanThreads) {
      const uint32_t b = b0 + tid;
      const uint32_t c = b < nblocks ? cnt[b] : 0, l = b < nblocks ? last[b] : 0;
      s_c[tid] = c; s_l[tid] = l;
      __syncthreads();
      for (int s = 1; s < kCsvScanThreads; s <<= 1) {
         const uint32_t yc = tid >= s ? s_c[tid - s] : 0, yl = tid >= s ? s_l[tid - s] : 0;
         __syncthreads();
         s_c[tid] += yc; s_l[tid] = yl > s_l[tid] ? yl : s_l[tid];
         __syncthreads(); }
      const uint32_t bc = s_carry_c, bl = s_carry_l;
      if (b < nblocks) {
         cnt[b] = bc + s_c[tid] - c;                                           // exclusive
         const uint32_t before = tid ? s_l[tid - 1] : 0;
         last[b] = before > bl ? before : bl; }
      __syncthreads();
      if (tid == kCsvScanThreads - 1) { s_carry_c = bc + s_c[tid]; s_carry_l = s_l[tid] > bl ? s_l[tid] : bl; }
      __syncthreads(); }
   if (tid == 0) {
      const uint32_t nl = s_carry_c, behind = s_carry_l;
      // fgets hands out an unterminated last line, and nothing for an empty one
      const bool tail = is_last && behind < nbytes;
      const long long lines = (long long)nl + (tail ? 1 : 0);
      starts[0] = 0;
      if (tail && lines <= starts_cap) starts[lines] = nbytes;
      rtfe_csv_window w;
      w.lines = lines; w.consumed = tail ? nbytes : behind;
      w.longest = tail ? nbytes - behind : 0;                                  // (k_csv_starts raises it)
      w.flags = lines > starts_cap ? RTFE_CSV_STARTS_FULL : 0;
      *out = w; } }

__global__ void __launch_bounds__(256) k_csv_starts(const uint4 *__restrict__ text, uint32_t nbytes, const uint32_t *__restrict__ boff, const uint32_t *__restrict__ bprev,
                                                    uint32_t *__restrict__ starts, long long starts_cap, rtfe_csv_window *__restrict__ out) {
   __shared__ uint32_t s_c[256], s_l[256];
   const int tid = threadIdx.x;
   const uint32_t chunk = blockIdx.x * 256u + tid;
   uint32_t m = csv_chunk_mask(text, nbytes, chunk);
   const uint32_t c = __popc(m), l = m ? chunk * kCsvLaneBytes + (32 - __clz((int)m)) : 0;
   s_c[tid] = c; s_l[tid] = l;
   __syncthreads();
   for (int s = 1; s < 256; s <<= 1) {
      const uint32_t yc = tid >= s ? s_c[tid - s] : 0, yl = tid >= s ? s_l[tid - s] : 0;
      __syncthreads();
      s_c[tid] += yc; s_l[tid] = yl > s_l[tid] ? yl : s_l[tid];
      __syncthreads(); }
   unsigned long long rank = (unsigned long long)boff[blockIdx.x] + s_c[tid] - c;      // newlines in front of this lane's chunk
   uint32_t open = tid ? s_l[tid - 1] : 0;                                       // where the line this chunk opens in starts
   const uint32_t bp = bprev[blockIdx.x];
   if (bp > open) open = bp;
   uint32_t longest = 0;
   while (m) {
      const uint32_t behind = chunk * kCsvLaneBytes + (uint32_t)__ffs((int)m);      // the offset behind this newline: the next line's first byte
      m &= m - 1;
      ++rank;
      if ((long long)rank <= starts_cap) starts[rank] = behind;
      const uint32_t len = behind - open;
      if (len > longest) longest = len;
      open = behind; }
   const int wl = csv_wave_max((int)(longest > 0x7fffffffu ? 0x7fffffffu : longest));
   if ((tid & 63) == 0 && wl > 0) atomicMax(reinterpret_cast<int *>(&out->longest), wl); }

// ---- the scanners of csrc/host/rt_csv.c on a line [p, e) of t ----
__device__ __forceinline__ int csv_at(const unsigned char *t, uint32_t p, uint32_t e) { return p < e ? (int)t[p] : 0; }

// scan_f64, the cursor only: the timestamp's value is the host's business (the first and the last surveyed line)
__device__ __forceinline__ void csv_skip_number(const unsigned char *t, uint32_t &p, uint32_t e) {
   int c = csv_at(t, p, e);
   while (c == ' ' || c == ',') c = csv_at(t, ++p, e);
   if (c == '-') c = csv_at(t, ++p, e);
   while (c >= '0' && c <= '9') c = csv_at(t, ++p, e);
   if (c == '.') {
      c = csv_at(t, ++p, e);
      while (c >= '0' && c <= '9') c = csv_at(t, ++p, e); } }

__device__ __forceinline__ float csv_scan_f32(const unsigned char *t, uint32_t &p, uint32_t e) {
   int c = csv_at(t, p, e);
   while (c == ' ' || c == ',') c = csv_at(t, ++p, e);
   const bool neg = c == '-';
   if (neg) c = csv_at(t, ++p, e);
   float v = 0;
   for (; c >= '0' && c <= '9'; c = csv_at(t, ++p, e)) v = v * 10 + (float)(c - '0');
   if (c == '.') {
      float scale = 10;
      for (c = csv_at(t, ++p, e); c >= '0' && c <= '9'; c = csv_at(t, ++p, e), scale *= 10) v += (float)(c - '0') / scale; }
   return neg ? -v : v; }

// (int) of a float as the host's cvttss2si gives it: what does not fit an int is INT_MIN.  Only a full scale of 0 or a value far outside it gets here;
// the rows stay the host loader's there too.
__device__ __forceinline__ int csv_to_int(float y) { return (y >= -2147483648.0f && y < 2147483648.0f) ? (int)y : (int)0x80000000; }

struct CsvParseArgs {
   const unsigned char *text; const uint32_t *starts;
   long long first_line, step, nkept;
   int ntrks, invert;
   float scale, maxvolts;
   unsigned long long perm_lo, perm_hi;      // the column of field k, 5 bits each: fields 0 .. 11 | 12 .. 18
   int16_t *rows; unsigned long long *clipped;
};

// where a wave finds its lines: from LDS if its span [the 16-byte boundary in front of its first line, the end of its last) fits the budget
// and the lines follow each other (step 1), where they lie otherwise.  Both give the same bytes.
struct CsvSpan { bool lds; uint32_t a0; };
__device__ __forceinline__ CsvSpan csv_stage(const unsigned char *text, const uint32_t *starts, long long first_line, long long step, long long n, uint4 *s_text) {
   const long long j0 = (long long)blockIdx.x * kCsvWaveLines;
   const long long j1 = j0 + kCsvWaveLines < n ? j0 + kCsvWaveLines : n;      // (a wave has at least one line: the grid is sized for that)
   CsvSpan sp; sp.lds = false; sp.a0 = 0;
   if (step != 1) return sp;
   const uint32_t a0 = starts[first_line + j0] & ~15u, e1 = starts[first_line + j1];
   if (e1 - a0 > (uint32_t)kCsvLdsBudget) return sp;
   const uint4 *src = reinterpret_cast<const uint4 *>(text + a0);
   const uint32_t nvec = (e1 - a0 + 15u) >> 4;
   for (uint32_t i = threadIdx.x; i < nvec; i += kCsvWaveLines) s_text[i] = src[i];
   __syncthreads();
   sp.lds = true; sp.a0 = a0;
   return sp; }

__device__ __forceinline__ float csv_line_peak(const unsigned char *t, uint32_t p, uint32_t e, int ntrks, float scale) {
   float peak = 0;
   csv_skip_number(t, p, e);
   for (int k = 0; k < ntrks; ++k) {
      float v = csv_scan_f32(t, p, e) * scale;
      if (v < 0) v = -v;
      if (peak < v) peak = v; }
   return peak; }

__global__ void __launch_bounds__(kCsvWaveLines) k_csv_peak(const unsigned char *__restrict__ text, const uint32_t *__restrict__ starts, long long first_line, long long nlines,
                                                            int ntrks, float scale, float *__restrict__ peak_out) {
   __shared__ uint4 s_text[kCsvLdsBudget / 16];
   const long long j = (long long)blockIdx.x * kCsvWaveLines + threadIdx.x;
   const CsvSpan sp = csv_stage(text, starts, first_line, 1, nlines, s_text);
   float peak = 0;
   if (j < nlines) {
      const uint32_t p = starts[first_line + j], e = starts[first_line + j + 1];
      peak = sp.lds ? csv_line_peak(reinterpret_cast<const unsigned char *>(s_text), p - sp.a0, e - sp.a0, ntrks, scale) : csv_line_peak(text, p, e, ntrks, scale); }
   // non-negative floats order as their bit patterns do: the maximum is exact whatever the order
   const int wm = csv_wave_max((int)__float_as_uint(peak));
   if ((threadIdx.x & 63) == 0 && wm > 0) atomicMax(reinterpret_cast<int *>(peak_out), wm); }

__device__ __forceinline__ int csv_line_row(const unsigned char *t, uint32_t p, uint32_t e, const CsvParseArgs &a, int16_t *o) {
   int clips = 0;
   csv_skip_number(t, p, e);
   for (int k = 0; k < a.ntrks; ++k) {
      const float v = csv_scan_f32(t, p, e) * a.scale;
      const int col = (int)((k < 12 ? a.perm_lo >> (5 * k) : a.perm_hi >> (5 * (k - 12))) & 31u);
      const float x = a.invert ? -v : v;
      int q = csv_to_int((x / a.maxvolts * 32767) + (x < 0 ? -0.5f : 0.5f));
      if (q <= -32767) { q = -32767; ++clips; }
      if (q >= 32767) { q = 32767; ++clips; }
      o[col] = (int16_t)q; }
   return clips; }

__global__ void __launch_bounds__(kCsvWaveLines) k_csv_parse(const CsvParseArgs a) {
   __shared__ uint4 s_text[kCsvLdsBudget / 16];
   const long long j = (long long)blockIdx.x * kCsvWaveLines + threadIdx.x;
   const CsvSpan sp = csv_stage(a.text, a.starts, a.first_line, a.step, a.nkept, s_text);
   int clips = 0;
   if (j < a.nkept) {
      const long long line = a.first_line + j * a.step;
      const uint32_t p = a.starts[line], e = a.starts[line + 1];
      int16_t *o = a.rows + j * a.ntrks;
      clips = sp.lds ? csv_line_row(reinterpret_cast<const unsigned char *>(s_text), p - sp.a0, e - sp.a0, a, o) : csv_line_row(a.text, p, e, a, o); }
   const int wc = csv_wave_sum(clips);
   if ((threadIdx.x & 63) == 0 && wc > 0) atomicAdd(a.clipped, (unsigned long long)wc); }

struct CsvGraphArgs {
   const unsigned char *text; const uint32_t *starts;
   long long first_line, step, nkept;
   int ntrks; float scale;
   long long first_sample, graphbin, nbins;
   int *bins, *peak;                          // non-negative floats, kept and compared as their bit patterns (k_csv_peak's argument)
};

// The converter's -graph (src/csvtbin.c:704-706, 719-722): kept line j is sample first_sample + j of the pass, and bins[that / graphbin] takes the line's
// max_k |field_k * scale|.  A wave's 64 samples are consecutive, so their bins ascend: where the first and the last agree (always, but for one wave per
// bin, once graphbin >= 64) the wave's maximum goes out in one atomic; otherwise a segmented scan leaves each run's maximum in its last lane.
__global__ void __launch_bounds__(kCsvWaveLines) k_csv_graph(const CsvGraphArgs a) {
   __shared__ uint4 s_text[kCsvLdsBudget / 16];
   const int lane = threadIdx.x & 63;
   const long long j0 = (long long)blockIdx.x * kCsvWaveLines, j = j0 + lane;
   const CsvSpan sp = csv_stage(a.text, a.starts, a.first_line, a.step, a.nkept, s_text);
   float v = 0;
   if (j < a.nkept) {
      const long long line = a.first_line + j * a.step;
      const uint32_t p = a.starts[line], e = a.starts[line + 1];
      v = sp.lds ? csv_line_peak(reinterpret_cast<const unsigned char *>(s_text), p - sp.a0, e - sp.a0, a.ntrks, a.scale) : csv_line_peak(a.text, p, e, a.ntrks, a.scale); }
   int bits = (int)__float_as_uint(v);
   const int wm = csv_wave_max(bits);
   if (a.peak && lane == 0 && wm > 0) atomicMax(a.peak, wm);
   // wave-uniform: the bins of the wave's first and last sample
   const long long jl = (j0 + kCsvWaveLines < a.nkept ? j0 + kCsvWaveLines : a.nkept) - 1;
   const long long b0 = (a.first_sample + j0) / a.graphbin, b1 = (a.first_sample + jl) / a.graphbin;
   if (b0 >= a.nbins) return;
   if (b0 == b1) {
      if (lane == 0 && wm > 0) atomicMax(a.bins + b0, wm);
      return; }
   // the lane's bin relative to b0 (r0 < graphbin, and r0 + 63 >= graphbin here); -1 for a lane without a line
   const long long r0 = a.first_sample + j0 - b0 * a.graphbin;
   int key = a.graphbin >= kCsvWaveLines ? (int)(r0 + lane >= a.graphbin) : (int)(((uint32_t)r0 + (uint32_t)lane) / (uint32_t)a.graphbin);
   if (j >= a.nkept) key = -1;
   for (int m = 1; m < kCsvWaveLines; m <<= 1) {
      const int src = lane >= m ? lane - m : lane;
      const int ob = __shfl(bits, src), ok = __shfl(key, src);
      if (lane >= m && ok == key && ob > bits) bits = ob; }
   const int next = __shfl(key, lane < kCsvWaveLines - 1 ? lane + 1 : lane);
   const bool tail = key >= 0 && (lane == kCsvWaveLines - 1 || next != key);
   if (tail && bits > 0 && b0 + key < a.nbins) atomicMax(a.bins + (b0 + key), bits); }

}  // namespace rtfe
