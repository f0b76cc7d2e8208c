// rtfe_textfile.hip — a SIMH .tap image in device memory -> the body of the interpreted text file (rtfe_text_format, include/rt_frontend.h).
//
// The text is the host writer's (csrc/host/rt_textfile.c, which restates src/textfile.c:228-275 for the terse layout of -tapread), byte for byte: per record a
// "%c%4d: " prefix, then lines of numbers (hex, octal, 16-bit octal words), blanks up to the character column, and the characters of one of thirteen codes;
// continuation lines start with seven blanks; a tape mark and the reader's messages are a line each.  The title and the trailer are the host's.
//
// What is parallel.  A line's BYTES are known without looking at the data - line k of a record is bytes [k * lse, (k + 1) * lse), lse = linesize (rounded up to
//   even under octal2, whose loop steps over pairs) - unless -linefeed is given.  Then a record falls into STRETCHES: one from its start, one from every 0x0a
//   (under octal2: at an even index; the odd ones are the second byte of a pair and are never tested), each cut into lines of lse on its own.  A 0x0a at index 0
//   leaves the prefix alone on a line: an empty first stretch.
//     k_tx_stretch   -linefeed only.  A wave per item: counts the stretches (ballots over 64 bytes at a time), and after a prefix sum over the items writes them,
//                    in order, into the stretch table.  Without -linefeed a stretch is an item and there is no table.
//     k_tx_measure   a lane per stretch: its lines.  Prefix sum: the first line of every stretch.
//     k_tx_len       a lane per line (binary search in that prefix sum): its length, from a table by the number of bytes in it (tail[], made by the host from the
//                    options) and the prefix's width.  One thing IS data dependent: with up to 7 tracks the reference prints a byte with "%02o", and a byte
//                    above 077 - a 7-track tape has none, but a .tap may hold anything, and -addparity makes them - takes a third digit; only then does this
//                    pass read data.  Sums per batch of lines, prefix sum: where each batch's text starts, the total, RTFE_TEXT_FULL.
//     k_tx_format    a workgroup is one wave and formats batches of `lines` consecutive lines, a lane a line, into LDS at the place each byte has in the text
//                    counted from the 16-byte boundary in front of the batch; the wave then copies whole aligned 16-byte vectors out and the at most two partial
//                    ones at its ends byte by byte (k_csvout_format's layout).  The code table in use (512 bytes: a character per byte value at an even and at an
//                    odd index - only the Flexowriter code tells them apart) is copied from the kernel's arguments into LDS once per workgroup.
//   The number of lines is known on the device only, so k_tx_len and k_tx_format run a fixed grid that strides over the batches.
//   Nothing is written at or behind text_cap, no table entry behind its table (RTFE_TEXT_SCRATCH_FULL), and the host has checked every item against the image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/rt_text_tables.h"
#include "rt_frontend.h"

namespace rtfe {

constexpr int kTxWave = 64;
constexpr int kTxLds = 16384;               // bytes of text a workgroup stages (with the code table nine workgroups share a CU's 160 KB): 64 lines of up to 255 bytes, at least 7 of the longest possible
constexpr int kTxScanThreads = 1024;
constexpr int kTxTail = RT_TEXT_MAXLINE + 2;
constexpr int kTxMaxGrid = 8192;

struct TxArgs {
   const unsigned char *image;
   const rtfe_text_item *items; long long nitems;
   int numtype, doboth, linesize, lse, dataspace, linefeed, narrow;
   int lines;                                // lines a batch
   unsigned long long max_stretches, max_batches;
   unsigned long long *cnt, *st, *lines_v, *base;      // scratch: stretches per item | the stretch table | lines per stretch | bytes per batch (all prefix-summed in place)
   unsigned long long *out_bytes, *out_lines, *out_stretches; uint32_t *out_flags;
   unsigned char *text; unsigned long long text_cap;
   uint16_t tail[kTxTail];                   // a line of n bytes behind its prefix: numbers, blanks, characters, '\n'
   unsigned char table[512];
};

__device__ static const char kTxMsg[3][40] = { RT_TAP_MARK_TEXT, "missing .tap end-of-medium marker\n", "erased gap\n" };

// ---- -linefeed: the stretches of every item ----
// entry: item << 32 | first << 31 | the index in the record at which it starts
template <bool kWrite> __global__ void __launch_bounds__(kTxWave) k_tx_stretch(const TxArgs a) {
   const int lane = threadIdx.x;
   const long long item = blockIdx.x;
   const rtfe_text_item it = a.items[item];
   const unsigned long long base = kWrite ? a.cnt[item] : 0, tag = (unsigned long long)item << 32;
   if (kWrite && lane == 0 && base < a.max_stretches) a.st[base] = tag | 1ull << 31;
   unsigned long long n = 1;
   if (it.kind == RT_TAP_RECORD) {
      const unsigned char *d = a.image + it.offset;
      const uint32_t L = it.length;
      for (uint32_t c0 = 0; c0 < L; c0 += kTxWave) {
         const uint32_t i = c0 + lane;
         const bool f = i < L && d[i] == 0x0a && (a.numtype != RT_NUM_OCTAL2 || (i & 1) == 0);
         const unsigned long long m = __ballot(f);
         if (kWrite && f) {
            const unsigned long long at = base + n + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
            if (at < a.max_stretches) a.st[at] = tag | i; }
         n += (unsigned long long)__popcll(m); } }
   if (!kWrite && lane == 0) a.cnt[item] = n; }

// in place: v[i] -> the sum in front of it, over n = n_host or ceil(*n_dev / div) values, at most n_max; the total; a flag where it is above limit.  One workgroup.
__global__ void __launch_bounds__(kTxScanThreads) k_tx_scan(unsigned long long *__restrict__ v, unsigned long long n_host, const unsigned long long *n_dev, unsigned long long div,
                                                            unsigned long long n_max, unsigned long long *total, unsigned long long limit, uint32_t *flags, uint32_t bit) {
   __shared__ unsigned long long s_v[kTxScanThreads];
   __shared__ unsigned long long s_carry;
   const int tid = threadIdx.x;
   unsigned long long n = n_dev ? (*n_dev + div - 1) / div : n_host;
   if (n > n_max) n = n_max;
   if (tid == 0) s_carry = 0;
   __syncthreads();
   for (unsigned long long b0 = 0; b0 < n; b0 += kTxScanThreads) {
      const unsigned long long b = b0 + tid;
      const unsigned long long x = b < n ? v[b] : 0;
      s_v[tid] = x;
      __syncthreads();
      for (int s = 1; s < kTxScanThreads; s <<= 1) {
         const unsigned long long y = tid >= s ? s_v[tid - s] : 0;
         __syncthreads();
         s_v[tid] += y;
         __syncthreads(); }
      const unsigned long long carry = s_carry;
      if (b < n) v[b] = carry + s_v[tid] - x;
      __syncthreads();
      if (tid == kTxScanThreads - 1) s_carry = carry + s_v[tid];
      __syncthreads(); }
   if (tid == 0) { *total = s_carry; if (flags && s_carry > limit) *flags |= bit; } }

__device__ __forceinline__ unsigned long long tx_nstretch(const TxArgs &a) {
   if (!a.linefeed) return (unsigned long long)a.nitems;
   const unsigned long long n = *a.out_stretches;
   return n < a.max_stretches ? n : a.max_stretches; }

struct TxStretch { long long item; uint32_t start, len; int first; };
__device__ __forceinline__ TxStretch tx_stretch(const TxArgs &a, unsigned long long s, unsigned long long ns) {
   TxStretch r;
   if (!a.linefeed) { r.item = (long long)s; r.start = 0; r.first = 1; r.len = a.items[s].kind == RT_TAP_RECORD ? a.items[s].length : 0; return r; }
   const unsigned long long e = a.st[s];
   r.item = (long long)(e >> 32); r.first = (int)((e >> 31) & 1); r.start = (uint32_t)(e & 0x7fffffffu);
   const rtfe_text_item it = a.items[r.item];
   r.len = it.kind == RT_TAP_RECORD ? it.length - r.start : 0;
   if (s + 1 < ns) { const unsigned long long e2 = a.st[s + 1]; if ((long long)(e2 >> 32) == r.item) r.len = (uint32_t)(e2 & 0x7fffffffu) - r.start; }
   return r; }

__global__ void __launch_bounds__(256) k_tx_measure(const TxArgs a) {
   const unsigned long long ns = tx_nstretch(a), s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
   if (s == 0 && !a.linefeed) *a.out_stretches = ns;
   if (s >= ns) return;
   const TxStretch r = tx_stretch(a, s, ns);
   a.lines_v[s] = r.len ? (r.len + (uint32_t)a.lse - 1) / (uint32_t)a.lse : 1; }

// ---- a line ----
struct TxLine { int msg; const unsigned char *d; uint32_t at, n, L; int head, err; };      // msg >= 0: kTxMsg[msg]; else bytes d[at .. at + n) of a record of L; head: the record's first line
__device__ __forceinline__ TxLine tx_line(const TxArgs &a, unsigned long long g, unsigned long long ns) {
   unsigned long long lo = 0, hi = ns;                                          // the last stretch whose first line is at or in front of g
   while (hi - lo > 1) { const unsigned long long mid = (lo + hi) >> 1; if (a.lines_v[mid] <= g) lo = mid; else hi = mid; }
   const TxStretch r = tx_stretch(a, lo, ns);
   const uint32_t k = (uint32_t)(g - a.lines_v[lo]);
   const rtfe_text_item it = a.items[r.item];
   TxLine l;
   l.msg = it.kind == RT_TAP_RECORD ? -1 : it.kind == RT_TAP_MARK ? 0 : 1 + (it.flag != 0);
   l.d = a.image + it.offset; l.L = it.length; l.err = it.flag != 0;
   l.at = r.start + k * (uint32_t)a.lse;
   const uint32_t left = r.len - k * (uint32_t)a.lse;
   l.n = left < (uint32_t)a.lse ? left : (uint32_t)a.lse;
   l.head = r.first && k == 0;
   return l; }

__device__ __forceinline__ int tx_prefix_width(uint32_t L) { return L < 10000u ? 7 : L < 100000u ? 8 : 9; }      // "%c%4d: "
// a byte printed alone with "%02o" that takes a third digit
__device__ __forceinline__ int tx_wide(const TxArgs &a, const TxLine &l) {
   if (!a.narrow || l.msg >= 0) return 0;
   if (a.numtype == RT_NUM_OCTAL) { int w = 0; for (uint32_t j = 0; j < l.n; ++j) w += l.d[l.at + j] > 077; return w; }
   if (a.numtype == RT_NUM_OCTAL2 && (l.n & 1)) return l.d[l.at + l.n - 1] > 077;
   return 0; }
__device__ __forceinline__ int tx_line_len(const TxArgs &a, const TxLine &l) {
   if (l.msg >= 0) { int n = 0; while (kTxMsg[l.msg][n]) ++n; return n; }
   return (l.head ? tx_prefix_width(l.L) : 7) + (int)a.tail[l.n] + tx_wide(a, l); }

__device__ __forceinline__ unsigned long long tx_nbatch(const TxArgs &a, unsigned long long nlines) {
   const unsigned long long nb = (nlines + (unsigned)a.lines - 1) / (unsigned)a.lines;
   return nb < a.max_batches ? nb : a.max_batches; }

__global__ void __launch_bounds__(kTxWave) k_tx_len(const TxArgs a) {
   const int lane = threadIdx.x;
   const unsigned long long ns = tx_nstretch(a), nlines = *a.out_lines, nb = tx_nbatch(a, nlines);
   for (unsigned long long b = blockIdx.x; b < nb; b += gridDim.x) {
      const unsigned long long g = b * (unsigned)a.lines + lane;
      int len = 0;
      if (lane < a.lines && g < nlines) len = tx_line_len(a, tx_line(a, g, ns));
      const int total = csv_wave_sum(len);
      if (lane == 0) a.base[b] = (unsigned long long)total; } }

// the line at o[0 ..] -> its length (tx_line_len's)
__device__ __forceinline__ int tx_put(const TxArgs &a, const TxLine &l, const unsigned char *tbl, unsigned char *o) {
   int p = 0;
   if (l.msg >= 0) { for (; kTxMsg[l.msg][p]; ++p) o[p] = (unsigned char)kTxMsg[l.msg][p]; return p; }
   if (l.head) {
      const int w = tx_prefix_width(l.L) - 3;
      o[p++] = l.err ? '!' : ' ';
      uint32_t v = l.L;
      for (int i = w - 1; i >= 0; --i) { o[p + i] = v || i == w - 1 ? (unsigned char)('0' + v % 10u) : ' '; v /= 10u; }
      p += w;
      o[p++] = ':'; o[p++] = ' '; }
   else for (int i = 0; i < 7; ++i) o[p++] = ' ';
   const unsigned char *d = l.d + l.at;
   const int n = (int)l.n;
   if (a.numtype == RT_NUM_NONE) { for (int j = 0; j < n; ++j) o[p++] = tbl[((l.at + j) & 1) * 256 + d[j]]; }
   else {
      for (int j = 0; j < n;) {
         const unsigned b = d[j];
         if (a.numtype == RT_NUM_HEX) { const unsigned h = b >> 4, q = b & 15; o[p++] = (unsigned char)(h < 10 ? '0' + h : 'A' + h - 10); o[p++] = (unsigned char)(q < 10 ? '0' + q : 'A' + q - 10); ++j; }
         else if (a.numtype == RT_NUM_OCTAL || l.at + j == l.L - 1) {
            if (!a.narrow || (b >> 6)) o[p++] = (unsigned char)('0' + (b >> 6));
            o[p++] = (unsigned char)('0' + ((b >> 3) & 7)); o[p++] = (unsigned char)('0' + (b & 7)); ++j; }
         else {
            const unsigned w = b << 8 | d[j + 1];
            for (int s = 15; s >= 0; s -= 3) o[p++] = (unsigned char)('0' + ((w >> s) & 7));
            j += 2; }
         if (a.dataspace > 0 && j % a.dataspace == 0) o[p++] = ' '; }
      if (a.doboth) {
         const int missing = a.linesize - n;
         int blanks = (a.dataspace ? missing / a.dataspace : 0) + missing * (a.numtype == RT_NUM_HEX || a.narrow ? 2 : 3);
         for (; blanks > 0; --blanks) o[p++] = ' ';
         if (a.dataspace == 0) { o[p++] = ' '; o[p++] = ' '; }
         for (int j = 0; j < n; ++j) o[p++] = tbl[((l.at + j) & 1) * 256 + d[j]]; } }
   o[p++] = '\n';
   return p; }

__global__ void __launch_bounds__(kTxWave) k_tx_format(const TxArgs a) {
   __shared__ uint4 s_text[kTxLds / 16];
   __shared__ unsigned char s_tbl[512];
   unsigned char *s = reinterpret_cast<unsigned char *>(s_text);
   const int lane = threadIdx.x;
   if (*a.out_flags & RTFE_TEXT_SCRATCH_FULL) return;                           // the stretch table is cut short: no text
   for (int i = lane; i < 512; i += kTxWave) s_tbl[i] = a.table[i];
   __syncthreads();
   const unsigned long long ns = tx_nstretch(a), nlines = *a.out_lines, nb = tx_nbatch(a, nlines);
   for (unsigned long long b = blockIdx.x; b < nb; b += gridDim.x) {
      const unsigned long long g = b * (unsigned)a.lines + lane;
      const bool active = lane < a.lines && g < nlines;
      TxLine l;
      int len = 0;
      if (active) { l = tx_line(a, g, ns); len = tx_line_len(a, l); }
      int incl = len;
      for (int dlt = 1; dlt < kTxWave; dlt <<= 1) { const int y = __shfl_up(incl, dlt); if (lane >= dlt) incl += y; }
      const unsigned long long lo = a.base[b], off = lo + (unsigned long long)(incl - len), e1 = lo + (unsigned long long)__shfl(incl, kTxWave - 1);
      const unsigned long long a0 = lo & ~15ull;
      if (active) tx_put(a, l, s_tbl, s + (off - a0));                          // (off - a0) + len <= 15 + lines * the longest possible line <= kTxLds
      __syncthreads();
      const unsigned long long end = e1 < a.text_cap ? e1 : a.text_cap;
      for (unsigned long long p = a0 + 16ull * lane; p < end; p += 16ull * kTxWave) {
         if (p >= lo && p + 16 <= end) *reinterpret_cast<uint4 *>(a.text + p) = s_text[(p - a0) >> 4];
         else {                                                                 // the vector holds a neighbouring batch's bytes too, or the cap cuts it
            const unsigned long long b0 = p > lo ? p : lo, b1 = p + 16 < end ? p + 16 : end;
            for (unsigned long long q = b0; q < b1; ++q) a.text[q] = s[q - a0]; } }
      __syncthreads(); } }

}  // namespace rtfe
