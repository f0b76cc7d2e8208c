// rtfe_api.hip — host side of the C ABI declared in include/rt_frontend.h (librtfe.so).
// Validates the configuration, derives window widths / thresholds exactly as the reference does
// (src/readtape.c:1402,1455-1457; src/decoder.c:448-449) and launches the kernels of a scan.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "rt_frontend.h"
#include "rtfe_device.h"

#include "rtfe_sift.hip"      // single translation unit: kernels + host API
#include "rtfe_kernels.hip"
#include "rtfe_zeros.hip"
#include "rtfe_diffz.hip"
#include "rtfe_ww.hip"
#include "rtfe_gain.hip"
#include "rtfe_dense.hip"
#include "rtfe_pack.hip"
#include "rtfe_csv.hip"
#include "rtfe_csvout.hip"
#include "rtfe_textfile.hip"
#include "rtfe_tapewrite.hip"

namespace rtfe {
__global__ void k_setup_exact(rtfe_burst *burst, BurstScratch *scratch, long long reset_row, long long end_row,
                              unsigned long long cap) {
   rtfe_burst b = {};
   b.zone_first = reset_row; b.zone_end = reset_row; b.reset_sample = reset_row; b.safe_last = reset_row;
   b.end_sample = end_row; b.event_base = 0; b.event_cap = (uint32_t)cap; b.flags = RTFE_F_EXACT_START;
   *burst = b;
   scratch->nbursts = 1; scratch->nbursts_total = 1; scratch->queue = 0; }
}  // namespace rtfe

using namespace rtfe;

constexpr int kGraphCache = 8;
struct rtfe_handle {
   rtfe_config cfg;
   DevCfg dev;
   DevCfg *d_dev;
   int lds_bytes;
   int num_cus;
   int timing;
   hipEvent_t (*ev0)[12], (*ev1)[12];    // timing: a ring of kTimingRing sets of start / stop events, a set per scan (on the stream it ran on)
   int ev_next, ev_pending;             // the set the next scan records into; sets recorded since rtfe_kernel_ms last looked
   unsigned ev_ran[64];                 // per set: the spans its scan ran (the others' events are recorded back to back and read 0, not the gap between two records)
   int zeros_kernel;                   // -zeros scans run k_zeros (RTFE_ZEROS_KERNEL=0: k_decode's zero-crossing mode, kept for tests)
   int diffz_kernel;                   // -zeros -differentiate scans run k_diffz (RTFE_DIFFZ_KERNEL=0: k_decode's walk_diffzeros, kept for tests)
   hipStream_t side;                   // the peak path's quiet map -> bursts -> restart rows beside its lists -> streams (both only need k_sift): RTFE_OVERLAP=0 keeps them in line
   hipEvent_t ev_fork, ev_join, ev_fork2, ev_join2;
   int overlap;
   int bursts_wpr;                     // RTFE_BURSTS_WPR: words of the quiet map per round of the zone search (tests: many rounds on a short tape); 0 = 4096
   int sfs_occ[kMaxScreens];           // k_sift_s: workgroups of a screen's instantiation a CU holds at once (the occupancy API, at create)
   long long work_cap;      // RTFE_WORK_CAP
   long long ccap_max;      // RTFE_CCAP (tests)
   long long seg_cap;       // RTFE_SEG_CAP (tests: a segment table that runs full); 0: sized from the streams
   int ds_order, dchain_wgs, prep_wgs, prep_run, dense_stop, dseg_wgs, dseg_threads;      // RTFE_DS_ORDER (0: chains in burst order), RTFE_DCHAIN_WGS / RTFE_PREP_WGS / RTFE_DSEG_WGS (workgroups per CU), RTFE_PREP_RUN (tiles a wave of k_prep), RTFE_DENSE_STOP (debugging): read once, at create
   int peak_stop, sift_wgs;                  // RTFE_PEAK_STOP (debugging: launch only the first n kernels of the peak path), RTFE_SIFT_WGS (k_sift's workgroups per CU, at most)
   int sift_generic, sift_per_screen, dseg_generic, tile_rows_set;      // RTFE_SIFT_GENERIC / RTFE_DSEG_GENERIC (the general kernels), RTFE_SIFT_PER_SCREEN=0, RTFE_TILE_ROWS given: the kernel pickers run at create (LDS limit, occupancy) and at every scan, and must decide alike
   // rtfe_set_graphs: a scan's launches (about twenty, on two streams) captured once per set of arguments into a HIP graph and replayed - what a scan of the same
   // buffers costs the host, and the gaps between its kernels on the device, shrink to one launch
   int graphs;
   struct GraphEnt { unsigned long long key[13]; hipGraphExec_t exec; unsigned long long stamp; } gcache[kGraphCache];
   unsigned long long gstamp;
};

static thread_local char g_err[512] = "";

static void drop_graphs(rtfe_handle *h) {
   for (int i = 0; i < kGraphCache; ++i) if (h->gcache[i].exec) { (void)hipGraphExecDestroy(h->gcache[i].exec); h->gcache[i].exec = nullptr; } }


// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the kernel on the CURRENT DEVICE, not of a handle: a second handle with a smaller LDS
// layout must not lower what a first one's launches need, a handle made on a second device must set it there too, and handles are made
// from several threads (ingest.py) - a table of the largest size asked for so far per (device, kernel), behind a mutex.
static void raise_dynamic_lds(const void *kernel, int bytes) {
   static std::mutex mu;
   static struct { const void *k; int dev, b; } seen[256];
   static int nseen = 0;
   int dev = 0;
   (void)hipGetDevice(&dev);
   std::lock_guard<std::mutex> lock(mu);
   for (int i = 0; i < nseen; ++i) if (seen[i].k == kernel && seen[i].dev == dev) {
      if (bytes > seen[i].b) seen[i].b = bytes;
      (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, seen[i].b); return; }
   if (nseen < 256) { seen[nseen].k = kernel; seen[nseen].dev = dev; seen[nseen].b = bytes; ++nseen; }
   (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); }
static int fail(int code, const char *fmt, ...) {
   va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
   return code; }

// the k_sift instantiation for a window width, a workgroup size and the vectors a thread prefetches
typedef void (*sf_kernel_t)(const DevCfg *, const int16_t *, long long, long long, uint16_t *, PeakDir *, unsigned char *, SfHard *, int, int *, unsigned long long *);
typedef void (*sfs_kernel_t)(const SfArgs);
constexpr int kSfWps = 5;          // waves per SIMD k_sift's register allocation is held to: four 5-wave workgroups per CU
constexpr int kSfsWps = 6;         // ... and k_sift_s': six four-wave workgroups per CU, 80 registers (round 6: 21.5 KB of LDS a workgroup - no staging slots - would let a seventh reside; at
                                   // 72 registers a prefetched vector spills, and the seventh workgroup is worth under 1 %: measured 0.6376 / 0.6428 ms)
template <int WM, int MAXT> static sf_kernel_t sf_kernel_nv(int nv) { return nv <= 4 ? k_sift<WM, MAXT, 4, kSfWps> : k_sift<WM, MAXT, 6, kSfWps>; }
template <int WM> static sf_kernel_t sf_kernel_t2(int threads, int nv) { return threads <= 320 ? sf_kernel_nv<WM, 320>(nv) : sf_kernel_nv<WM, 640>(nv); }
static sf_kernel_t sf_kernel(int wmax, int threads, int nv) {
   return wmax <= 18 ? sf_kernel_t2<18>(threads, nv) : sf_kernel_t2<50>(threads, nv); }
// one screen of a width and a track count the lean kernel is built for, a sure level that fits 16 bits: k_sift_s
template <int NT, bool PL> static sfs_kernel_t sfs_kernel_w(int w) {
   switch (w) {
      case 6:  return k_sift_s<6, NT, kSfsWps, PL>;
      case 7:  return k_sift_s<7, NT, kSfsWps, PL>;
      case 8:  return k_sift_s<8, NT, kSfsWps, PL>;
      case 9:  return k_sift_s<9, NT, kSfsWps, PL>;
      case 10: return k_sift_s<10, NT, kSfsWps, PL>;
      case 11: return k_sift_s<11, NT, kSfsWps, PL>;
      case 12: return k_sift_s<12, NT, kSfsWps, PL>;
      case 13: return k_sift_s<13, NT, kSfsWps, PL>;
      case 14: return k_sift_s<14, NT, kSfsWps, PL>;
      case 15: return k_sift_s<15, NT, kSfsWps, PL>;
      case 16: return k_sift_s<16, NT, kSfsWps, PL>;
      case 17: return k_sift_s<17, NT, kSfsWps, PL>;
      default: return nullptr; } }
// (every window width the packed derivation holds - 6 .. 17 samples - for nine and seven tracks: 800 / 556 BPI NRZI at 781 kHz are 13 / 19,
//  at half that rate 6 / 9; wider windows, several widths and other track counts take the general kernel: 2.1 instead of 0.93 ms on C2)
static sfs_kernel_t sfs_kernel(int w, int ntrks, bool plain) {
   if (plain) return ntrks == 9 ? sfs_kernel_w<9, true>(w) : (ntrks == 7 ? sfs_kernel_w<7, true>(w) : nullptr);
   return ntrks == 9 ? sfs_kernel_w<9, false>(w) : (ntrks == 7 ? sfs_kernel_w<7, false>(w) : nullptr); }
// k_dseg with the track count at compile time for the usual tapes
typedef void (*ds_kernel_t)(const DevCfg *, const int16_t *, long long, long long, unsigned char *, unsigned char *, unsigned char *, unsigned long long *);
static ds_kernel_t ds_kernel(const rtfe_handle *h) { return h->dseg_generic ? k_dseg<0> : (h->dev.ntrks == 9 ? k_dseg<9> : (h->dev.ntrks == 7 ? k_dseg<7> : k_dseg<0>)); }
// k_zeros with the track count at compile time for the usual tapes
typedef void (*zeros_kernel_t)(const DevCfg *, const int16_t *, long long, long long, rtfe_burst *, BurstScratch *, uint32_t *, rtfe_event *);
static zeros_kernel_t zeros_kernel(int ntrks) { return ntrks == 9 ? k_zeros<9> : (ntrks == 7 ? k_zeros<7> : k_zeros<0>); }
static int sf_wmax(const DevCfg &d) { int w = 0; for (int s = 0; s < d.nscreens; ++s) if (d.screen[s].W > w) w = d.screen[s].W; return w; }
static int sf_threads(const DevCfg &d) { return 64 * ((d.ntrks + 1) / 2); }
static int sf_nvec(const DevCfg &d) { return (d.pk_hl + kSfTile + d.pk_hr) * d.ntrks / 8; }
static int sf_nv(const DevCfg &d) { return (sf_nvec(d) + sf_threads(d) - 1) / sf_threads(d); }
// (several window widths - a parameter sweep -: a launch of the lean kernel per screen, if every screen has one: NRZI -m is three widths, 1.5 ms each where the
//  general kernel's loop over the screens took 15.8)
static sfs_kernel_t sf_special_sc(const rtfe_handle *h, int sc) {
   const DevCfg &d = h->dev;
   return (d.screen[sc].sure_i <= 32767 && !h->sift_generic) ? sfs_kernel(d.screen[sc].W, d.ntrks, d.pk_plain != 0) : nullptr; }
static sfs_kernel_t sf_special(const rtfe_handle *h) {
   const DevCfg &d = h->dev;
   if (d.nscreens > 1 && !h->sift_per_screen) return nullptr;
   for (int sc = 0; sc < d.nscreens; ++sc) if (!sf_special_sc(h, sc)) return nullptr;
   return d.nscreens >= 1 ? sf_special_sc(h, 0) : nullptr; }
// k_sift_s has a geometry of its own: a wave per pair of heads with an odd last head's tile split among them, only the window's rows in front of a tile
static int sfs_threads(const DevCfg &d) { return 64 * sfs_waves(d.ntrks); }
static int sfs_lds_sc(const DevCfg &d, int sc) { return (int)sfs_lds_layout(d.ntrks, d.screen[sc].W, d.pk_wave_cap, d.pk_slot).total + 64; }
static int sfs_lds(const DevCfg &d) { int m = 0; for (int sc = 0; sc < d.nscreens; ++sc) { const int v = sfs_lds_sc(d, sc); if (v > m) m = v; } return m; }

extern "C" int rtfe_abi_version(void) { return RTFE_ABI_VERSION; }
extern "C" const char *rtfe_last_error(void) { return g_err; }

// The timed spans of one rtfe_scan (rtfe_kernel_ms), in launch order.  The peak path (NRZI peak detection) runs
//   k_sift | k_prep [k_sift_hard, k_pscan1/2, k_prep] beside k_bursts [k_qpack, k_bursts, k_zones: on a stream of the handle's own] | k_gain [the chains' heads] | k_gain_s [k_gain_seg, k_gain_join] |
//   k_gain_tail | k_emit [k_emit_seg, k_emit, k_publish] | k_decode [the bursts the chains gave up, on the samples]
// the sample path (PE, GCR, differentiated peaks, density detection, parameter-set sweeps with too many widths) k_quiet | k_bursts | k_decode,
// -zeros k_quiet | k_bursts | k_zeros, -zeros -differentiate k_quiet | k_bursts | k_diffz (timed in the k_zeros span).  A span a scan does not run reads 0.
// the dense sample path (PE, GCR peak detection): k_dseg [quiet map folded in] | k_bursts [k_bursts, k_zones] | k_dchain [k_dorder, k_dchain, k_publish] | k_decode [what the chains gave up]
static const char *KNAMES[] = {"k_quiet", "k_sift", "k_prep", "k_bursts", "k_gain", "k_gain_s", "k_gain_tail", "k_emit", "k_decode", "k_zeros", "k_dseg", "k_dchain"};
enum { kTQuiet, kTSift, kTPrep, kTBursts, kTGain, kTGainS, kTGainTail, kTEmit, kTDecode, kTZeros, kTDseg, kTDchain };
constexpr int kNumKernels = 12;
static_assert(kNumKernels <= 12, "rtfe_handle::ev0 / ev1 hold 12 events a set");
extern "C" int rtfe_kernel_count(void) { return kNumKernels; }
extern "C" const char *rtfe_kernel_name(int i) { return (i >= 0 && i < kNumKernels) ? KNAMES[i] : ""; }

static int create_impl(const rtfe_config *c, rtfe_handle **out, int tile_override);
// workgroups a CU's 160 KB of LDS hold: `slack` bytes a workgroup for its static part and the allocation granularity, at most `cap` (a caller's knob and
// the floor of one come behind it)
static int lds_wgs_per_cu(int lds, int slack, int cap) { const int n = (160 * 1024) / (lds + slack); return n < cap ? n : cap; }

// k_decode's launch.  One wave per 64 walkers: the walk phase is latency bound, so small workgroups (many resident per CU) beat wide ones; it holds
// ~250 VGPRs => 2 waves/SIMD => 8 waves per CU.  rtfe_create's choice of the tile size, rtfe_scan's grid and rtfe_scan_exact's workgroup all come from here.
struct DecodePlan { int walker_threads, threads, per_cu; };      // (walker_threads: rtfe_scan_exact's single workgroup, a lane per walker)
static DecodePlan decode_plan(const rtfe_handle *h) {
   DecodePlan p;
   const int nwalk = h->dev.nparm * h->dev.ntrks;
   p.walker_threads = p.threads = nwalk <= 64 ? 64 : (nwalk <= 128 ? 128 : 256);
   if (h->dev.find_zeros && !h->dev.differentiate) {                 // -zeros through k_decode (rtfe_zeros.hip says when): a lane per (track, 64-row sub-segment) of the tile
      const int lanes = h->dev.ntrks * (h->dev.tile_rows / 64);
      while (p.threads < lanes && p.threads < 256) p.threads *= 2; }
   p.per_cu = lds_wgs_per_cu(h->lds_bytes, 1024, 8 / (p.threads / 64));
   if (p.per_cu < 1) p.per_cu = 1;
   return p; }

extern "C" int rtfe_create(const rtfe_config *c, rtfe_handle **out) {
   if (!c || !out) return fail(-1, "null argument");
   rtfe_handle *h = nullptr;
   int rc = create_impl(c, &h, 0);
   if (rc != 0) return rc;
   // The sample path (PE, GCR, parameter-set sweeps with several window widths) keeps a tile, its screen maps and its walkers in
   // LDS: with 512-row tiles a sweep's workgroup can be the only one on its CU.  Shorter tiles that let more workgroups reside win
   // (C4: 98 KB -> 75 KB, one -> two per CU, +35 %); the peak path and -zeros have their own tile sizes.
   // (only then: where several workgroups already share a CU the longer tile is better - GCR, one set: 18.4 vs 22.9 ms per 5e7 rows)
   if (!h->tile_rows_set && !h->dev.find_zeros && h->dev.mode != RTFE_WW && decode_plan(h).per_cu == 1) {
      rtfe_handle *h2 = nullptr;
      if (create_impl(c, &h2, kMarginRows) == 0) {
         if (decode_plan(h2).per_cu > decode_plan(h).per_cu) { rtfe_destroy(h); h = h2; }
         else rtfe_destroy(h2); } }
   *out = h;
   return 0; }

static int create_impl(const rtfe_config *c, rtfe_handle **out, int tile_override) {
   if (c->ntrks < 1 || c->ntrks > RTFE_MAXTRKS) return fail(-2, "ntrks %d out of range", c->ntrks);
   if (c->mode != RTFE_NRZI && c->mode != RTFE_PE && c->mode != RTFE_GCR && c->mode != RTFE_WW)
      return fail(-3, "mode %d not known", c->mode);
   if (c->mode == RTFE_WW && c->nparmsets != 1)
      return fail(-3, "Whirlwind: one parameter set (rtfe_ww_scan; with -zeros / -differentiate rtfe_ww_detector_scan)");
   if (c->nparmsets < 1 || c->nparmsets > RTFE_MAXPARMSETS) return fail(-5, "nparmsets %d out of range", c->nparmsets);
   if (c->nparmsets * c->ntrks > kDecodeThreads) return fail(-6, "nparmsets*ntrks > %d", kDecodeThreads);
   if (!(c->bpi >= 0) || !(c->ips > 0) || c->tdelta_ns <= 0 || !(c->maxvolts > 0)) return fail(-7, "ips, tdelta_ns and maxvolts must be positive, bpi >= 0");
   // bpi == 0: the density is unknown - the front end of the reference's density pre-pass (src/readtape.c:1656-1672):
   // window of 8 samples, no AGC / baseline feedback (no decoder runs).  Sizing heuristics then assume 12 samples per bit.
   const bool density_mode = c->bpi == 0;
   if (density_mode && (c->find_zeros || c->mode != RTFE_NRZI)) return fail(-7, "bpi = 0 (density detection) is built for the NRZI peak detector only");
   const float bpi_s = density_mode ? 1.0f / (c->ips * ((float)c->tdelta_ns / 1e9f) * 12.0f) : c->bpi;
   rtfe_handle *h = new rtfe_handle();
   h->cfg = *c;
   h->timing = 0; h->ev0 = nullptr; h->ev1 = nullptr; h->ev_next = 0; h->ev_pending = 0; memset(h->ev_ran, 0, sizeof h->ev_ran);
   DevCfg &d = h->dev;
   memset(&d, 0, sizeof d);
   d.mode = c->mode; d.ntrks = c->ntrks; d.invert = c->invert != 0; d.nparm = c->nparmsets;
   d.find_zeros = c->find_zeros != 0;
   d.differentiate = c->differentiate != 0;
   d.agc_off = density_mode;
   bool seen[RTFE_MAXTRKS] = {false};
   for (int i = 0; i < c->ntrks; ++i) {
      int t = c->head_to_trk[i];
      if (t < 0 || t >= c->ntrks || seen[t]) { delete h; return fail(-8, "head_to_trk is not a permutation"); }
      seen[t] = true; d.head_to_trk[i] = t; d.trk_to_head[t] = i;
      int s = c->skew_delaycnt[i];
      if (s < 0 || s > 50) { delete h; return fail(-9, "skew %d out of range 0..50 (MAXSKEWSAMP)", s); }
      d.skew[i] = s; if (s > d.maxskew) d.maxskew = s; }
   d.maxvolts = c->maxvolts;
   d.sample_deltat = (float)c->tdelta_ns / 1e9f;                       // src/readtape.c:1345
   d.tdelta_ns = c->tdelta_ns; d.tstart_ns = c->tstart_ns;
   const float bitspace = density_mode ? 0.0f : 1 / (c->bpi * c->ips);  // src/decoder.c:448 (not initialised during density detection)
   const float hfloor = c->screen_floor_height > 0 ? c->screen_floor_height : 1.0f;
   const double lsb_per_volt = 32767.0 / (double)c->maxvolts;
   float quiet_v = 1e9f;
   for (int p = 0; p < c->nparmsets; ++p) {
      const rtfe_parmset &ps = c->parmset[p];
      DevParm &dp = d.parm[p];
      int W = density_mode ? 8 : (int)(ps.pkww_bitfrac / (c->bpi * c->ips * d.sample_deltat));     // src/readtape.c:1455-1457
      if (W > 50) W = 50;
      if (W < 2) { delete h; return fail(-10, "parmset %d: window of %d samples is too small", p, W); }
      if (ps.agc_window < 0 || ps.agc_window > 10) { delete h; return fail(-11, "parmset %d: agc_window out of range", p); }
      if (ps.agc_window && ps.agc_alpha != 0) { delete h; return fail(-12, "parmset %d: inconsistent AGC parameters", p); }   // src/decoder.c:502
      dp.W = W; dp.rise = ps.pkww_rise; dp.min_peak = ps.min_peak; dp.agc_alpha = ps.agc_alpha; dp.agc_window = ps.agc_window;
      dp.t_clkwindow = bitspace / 2 * ps.clk_factor;                      // src/decoder.c:449
      int s;
      for (s = 0; s < d.nscreens; ++s) if (d.screen[s].W == W) break;
      if (s == d.nscreens) {
         if (s == kMaxScreens) { delete h; return fail(-13, "more than %d distinct window widths", kMaxScreens); }
         d.screen[s].W = W; d.screen[s].rise_i = 1 << 30; d.screen[s].minpk_i = 1 << 30; ++d.nscreens; }
      dp.screen = s;
      // dead-quiet band: no detection is possible from a freshly reset detector (agc 1, baseline 4 V) while
      // |v| < min_peak, or while the signal range 2|v| < pkww_rise
      float q = ps.min_peak > ps.pkww_rise / 2 ? ps.min_peak : ps.pkww_rise / 2;
      if (q < quiet_v) quiet_v = q; }
   // the candidate screens: the loosest thresholds the AGC can ever ask for, given v_avg_height >= hfloor and agc_gain <= 2 (screen_thresholds, rtfe_kernels.hip).
   // A floor the caller gave stands; the default (1 V: every tape clears it) is where the handle starts, and behind each scan of the peak path the
   // floor moves to half the smallest peak height the scan's chains learned (k_adapt_floor; RTFE_ADAPT_FLOOR=0: never)
   d.floor_cfg = hfloor; d.floor_probed = 0; d.probe_min = 0x7fffffff; d.probe_ticket = 0;
   d.probe_on = !(getenv("RTFE_FLOOR_PROBE") && atoi(getenv("RTFE_FLOOR_PROBE")) == 0);
   d.adapt_floor = !(c->screen_floor_height > 0) && !(getenv("RTFE_ADAPT_FLOOR") && atoi(getenv("RTFE_ADAPT_FLOOR")) == 0);
   screen_thresholds(d, hfloor);
   // k_peaks: a row whose margin reaches sure_i passes the rise test for every threshold the chains accept without asking
   // (tightest: baseline 1.5 x full scale at half gain); k_chain hands a burst whose threshold climbs beyond that to the sample path
   for (int s = 0; s < d.nscreens; ++s) {
      float hi_v = 0;
      for (int p = 0; p < c->nparmsets; ++p) if (d.parm[p].screen == s) { const float v = c->parmset[p].pkww_rise * (1.5f * c->maxvolts / 4.0f) / 0.5f; if (v > hi_v) hi_v = v; }
      long long si = (long long)ceil((double)hi_v * lsb_per_volt) + 3;
      if (si > 65535) si = 65535;
      if (si <= d.screen[s].rise_i + 1) si = d.screen[s].rise_i + 2;
      d.screen[s].sure_i = (int)si; }
   if (d.find_zeros) {
      // the zero-crossing detector has no amplitude feedback and no parameter-set dependence (adjust_agc returns
      // at once, src/decoder.c:501): one walker per track; nothing can become pending while |v| <= 0.2 V
      quiet_v = 0.2f;
      d.samples_per_bit = (int)(1 / (bpi_s * c->ips * d.sample_deltat));          // src/readtape.c:1402
      // differentiated: a restart differentiates against 0 and consecutive samples differ by up to 2q, and neither
      // may reach 0.2 V after the x0.4 x samples_per_bit scaling (src/readtape.c:1388)
      if (d.differentiate) quiet_v = 0.24f / (float)(d.samples_per_bit > 0 ? d.samples_per_bit : 1);
      // P = the smallest c in 1 .. 32768 with volt(c) > 0.2 V (exact, same expression as the device's volt(); monotone in c, and
      // volt(-c) = -volt(c)): a top confirms at v >= P, a bottom at v <= -P.  32768 counts: -32768 is a sample (and -invert turns it
      // into +32768).  P = 32768 (maxvolts just under 0.2 V .. 0.2 V): only -32768 can confirm; P = 32769: nothing can.  Either way
      // k_zeros' 16-bit lanes cannot hold P and k_decode's 32-bit mode takes the scan
      int code = 1;
      while (code <= 32768 && !((float)code / 32767 * c->maxvolts > 0.2f)) ++code;
      d.zc_peak_i = code; }
   if (d.differentiate && !d.find_zeros) {
      // peak detection on the differentiated signal (src/readtape.c:1383-1394): a zone is safe where the dead band
      // (|delta| < 0.05 V -> 0) makes the detector's input exact zeros: |v| < 0.024 V covers both the restart (delta
      // against 0) and consecutive samples.  No candidate screen runs in this mode.
      if (quiet_v > 0.024f) quiet_v = 0.024f;
      d.samples_per_bit = (int)(1 / (bpi_s * c->ips * d.sample_deltat));          // src/readtape.c:1402
      for (int p = 0; p < c->nparmsets; ++p) { d.parm[p].screen_rise_v = -1; d.parm[p].screen_minpk_v = -1; } }
   if (c->quiet_volts > 0 && c->quiet_volts < quiet_v) quiet_v = c->quiet_volts;
   d.quiet_i = (int)floor(quiet_v * 0.98 * lsb_per_volt) - 1;
   if (d.quiet_i < 0) d.quiet_i = 0;
   const int spb = (int)(1 / (bpi_s * c->ips * d.sample_deltat));
   int gap = c->gap_min_samples > 0 ? c->gap_min_samples : 32 * (spb > 0 ? spb : 1);
   if (gap < kMarginRows + 128) gap = kMarginRows + 128;
   d.gap_chunks = (gap + kChunkRows - 1) / kChunkRows + 1;                 // quiet-map chunks are groups of 64 rows
   d.zc_parallel = 1;
   if (const char *e = getenv("RTFE_ZC_PARALLEL")) d.zc_parallel = atoi(e) != 0;
   {  // rows a -zeros sub-segment starts early from a fresh state: two bit cells hold a confirmed crossing in each direction wherever
      // the signal is live; where that is not enough the join check sees it and the sub-segment is run again (exact either way)
      const float spbw = (bpi_s > 0 && c->ips > 0) ? 1.0f / (bpi_s * c->ips * d.sample_deltat) : 32.0f;
      int w = ((int)(2.0f * spbw) + 7) & ~7;
      d.zc_warm = w < 16 ? 16 : (w > 64 ? 64 : w); }
   if (const char *e = getenv("RTFE_ZC_WARM")) { const int v = atoi(e) & ~7; if (v >= 8 && v <= 64) d.zc_warm = v; }
   d.tail_rows = 48 * (spb > 0 ? spb : 1);                              // 48 bit cells of silence: every format has ended its block (NRZI ~10, PE 2.5, GCR 6)
   if (const char *e = getenv("RTFE_TAIL_ROWS")) d.tail_rows = atoi(e);   // (tests: 0 = walk the whole gap)
   d.cap_frac = c->events_per_sample_cap > 0 ? c->events_per_sample_cap : 0.125f;
   {
      const char *e = getenv("RTFE_TILE_ROWS");            // tuning knob; the default is what bench.py measures
      h->tile_rows_set = e != nullptr;
      // (-zeros in k_decode's zero-crossing mode - k_zeros does not tile -: a lane per (track, 64-row sub-segment), 14 sub-segments x 9 tracks fill two waves)
      int tr = tile_override > 0 ? tile_override : (e ? atoi(e) : ((c->find_zeros && !c->differentiate) ? 64 * (128 / (c->ntrks > 0 ? c->ntrks : 9)) : 512));
      tr = (tr / 64) * 64;
      if (tr < kMarginRows) tr = kMarginRows;
      if (tr > kMaxTileRows) tr = kMaxTileRows;
      d.tile_rows = tr; }
   {
      int wmax = 0;
      for (int sidx = 0; sidx < d.nscreens; ++sidx) if (d.screen[sidx].W > wmax) wmax = d.screen[sidx].W;
      d.halo_rows = (kScreenHalo + wmax + 1 + d.maxskew + 7) & ~7;
      if (d.halo_rows > kMaxHaloRows) d.halo_rows = kMaxHaloRows;
      d.ldw = d.halo_rows + d.tile_rows + 8; }
   d.lsb_per_volt = (float)(32767.0 / (double)c->maxvolts);
   d.debug = getenv("RTFE_DEBUG") ? atoi(getenv("RTFE_DEBUG")) : 0;
   d.cut = getenv("RTFE_CUT") ? atoi(getenv("RTFE_CUT")) : 0;
   // (k_sift_s's plain build: none of the knobs it would otherwise carry as run-time values; RTFE_SIFT_PLAIN=0: the general build everywhere - tests)
   d.pk_plain = !d.invert && d.cut == 0 && d.debug != 3 && !(getenv("RTFE_SIFT_PLAIN") && atoi(getenv("RTFE_SIFT_PLAIN")) == 0);
   {  // The peak path (k_sift -> k_gain -> k_emit): peak detection on the undifferentiated signal.  It pays where flux transitions are a
      // bit cell apart (NRZI): most peaks then have the window to themselves and the chains stay on their steady path.  PE and GCR put
      // a top and a bottom into one window; their bursts take the sample path (k_decode) - RTFE_PEAK_PATH=0/1 overrides (tests keep both
      // paths covered for every format).
      d.peak_path = !d.find_zeros && !d.differentiate && d.mode == RTFE_NRZI;
      if (const char *e = getenv("RTFE_PEAK_PATH")) d.peak_path = !d.find_zeros && !d.differentiate && d.mode != RTFE_WW && atoi(e) != 0;
      d.pk_fast = 1;
      if (const char *e = getenv("RTFE_GAIN_FAST")) d.pk_fast = atoi(e) != 0;
      // the chains' steady stretches in segments (k_gain_seg): 256 records each (measured on C2: 64 / 128 / 256 -> 2.61 / 2.43 / 2.39 ms per scan); the warm-up from the alpha filter's memory
      d.pk_seg_recs = 256;
      d.pk_mar = kPkMar;
      if (const char *e = getenv("RTFE_PK_MAR")) { const int v = atoi(e); if (v >= 0 && v <= kPkMar) d.pk_mar = v; }      // (tests: margins from the samples)
      if (const char *e = getenv("RTFE_SEG_RECS")) { const int v = atoi(e) & ~7; if (v >= 8 && v <= 4096) d.pk_seg_recs = v; }
      d.pk_rejoin = getenv("RTFE_SEG_REJOIN") ? atoi(getenv("RTFE_SEG_REJOIN")) != 0 : 1;      // (0: a chain that breaks is walked to its end by one lane, as before round 5's last part; tests)
      for (int p = 0; p < c->nparmsets; ++p) {
         const float a = c->parmset[p].agc_alpha;
         // (1 - alpha)^n < 2^-26 brings two gains within an ulp; 64 records more for the last ulp to collapse under the filter's own
         // rounding (round 2 measured the same on the old walk: ~50 records left 3 % of the joins a few ulps apart, ~200 none in 8 000)
         int wm = ((a > 0 && a < 1) ? (int)ceil(log(1.0 / 67108864.0) / log(1.0 - (double)a)) : 16) + 64;
         wm = wm > 1024 ? 1024 : wm;
         if (const char *e = getenv("RTFE_SEG_WARM")) { const int v = atoi(e); if (v >= 0 && v <= 4096) wm = v; }
         d.parm[p].seg_warm = wm; }
      const int wmax = sf_wmax(d);
      d.pk_hl = (kPkBack + 2 * wmax + 6 + 7) & ~7;
      d.pk_hr = (wmax + 2 + 7) & ~7;
      // pool slots: flux transitions per tile and head from the bit cell (PE: up to two per cell), 16 bytes each (a record and its margin
      // block), half as much again for noise and weak peaks.  RTFE_PK_SLOT: tests force the capacity path.
      const float spbf = 1.0f / (bpi_s * c->ips * d.sample_deltat);
      const float ppb = c->mode == RTFE_PE ? 2.0f : 1.0f;
      int slot = (int)((float)kSfTile / (spbf > 2 ? spbf : 2) * ppb * 16.0f * 1.5f) + 160;
      // a screen below the noise floor - no amplitude test, or one as low as the rise test: noise wiggles become runs, every row explicit
      bool noisy_screen = false;
      for (int sidx = 0; sidx < d.nscreens; ++sidx) {
         const bool rise_low = (double)d.screen[sidx].rise_i / lsb_per_volt < 0.03, amp_low = d.screen[sidx].minpk_i < 0 || (double)d.screen[sidx].minpk_i / lsb_per_volt < 0.03;
         if (rise_low && amp_low) noisy_screen = true; }
      if (noisy_screen) slot *= 3;
      d.pk_wave_cap = noisy_screen ? 1792 : (getenv("RTFE_PK_WAVECAP") ? atoi(getenv("RTFE_PK_WAVECAP")) : 384);                          // (a wave's two heads have 2 x 896 samples)
      if (const char *e = getenv("RTFE_PK_SLOT")) { const int v = atoi(e); if (v >= 32 && v <= 65536) slot = v; }
      d.pk_slot = (slot + 15) & ~15;
      d.pk_lds = (int)sf_lds_layout(c->ntrks, d.pk_hl, d.pk_hr, d.pk_wave_cap, d.pk_slot).total + 64;
      if (d.pk_lds > 150 * 1024 || sf_nv(d) > 6) d.peak_path = 0; }
   {  // ---- the dense sample path (rtfe_dense.hip) ----
      // parameter sets the front end cannot tell apart are one chain (src/parmsets.c:77-110: four of the five GCR defaults, five of the eight PE ones)
      d.nuset = 0;
      for (int p = 0; p < c->nparmsets; ++p) {
         int u;
         for (u = 0; u < d.nuset; ++u) {
            const DevParm &a = d.parm[d.uset_rep[u]], &b = d.parm[p];
            if (a.W == b.W && a.rise == b.rise && a.min_peak == b.min_peak && a.agc_alpha == b.agc_alpha && a.agc_window == b.agc_window
                && (c->mode != RTFE_PE || a.t_clkwindow == b.t_clkwindow)) break; }
         if (u == d.nuset) { d.uset_rep[u] = p; d.uset_mask[u] = 0; ++d.nuset; }
         d.uset_of[p] = u; d.uset_mask[u] |= 1u << p; }
      if (getenv("RTFE_DENSE_DEDUP") && atoi(getenv("RTFE_DENSE_DEDUP")) == 0) {      // (tests: every set its own chain)
         d.nuset = c->nparmsets;
         for (int p = 0; p < c->nparmsets; ++p) { d.uset_of[p] = p; d.uset_rep[p] = p; d.uset_mask[p] = 1u << p; } }
      // The default for PE and GCR peak detection (round 4): measured against k_decode on 1e7 .. 2.7e8 rows it is 1.05 - 2.4 x faster (DESIGN.md 4d;
      // most where several parameter sets share a window width); RTFE_DENSE_PATH=0 keeps k_decode (the tests run both against each other)
      d.dense_path = !d.peak_path && !d.find_zeros && !d.differentiate && !d.agc_off && (d.mode == RTFE_PE || d.mode == RTFE_GCR);
      if (const char *e = getenv("RTFE_DENSE_PATH")) d.dense_path = !d.peak_path && !d.find_zeros && !d.differentiate && !d.agc_off && d.mode != RTFE_WW && atoi(e) != 0;
      int wpad = 64;
      for (int sidx = 0; sidx < d.nscreens; ++sidx) {
         // (two windows and a little: a lane's warm-up only has to see one detection the true chain sees too; the join checks that it did -
         //  measured on C4: 74 -> 60 rows makes k_dseg 9 % faster and 0.4 % more joins fail)
         int wm = 2 * d.screen[sidx].W + 16; if (wm < 48) wm = 48;
         if (const char *e = getenv("RTFE_DS_WARM")) { const int v = atoi(e); if (v >= 0 && v <= 192) wm = v; }      // (tests: joins that fail)
         d.ds_warm[sidx] = wm; if (wm > wpad) wpad = wm; }
      d.ds_pad = (wpad + 63) & ~63;
      const float spbf = 1.0f / (bpi_s * c->ips * d.sample_deltat);
      const float expect = (float)kDsSub * (c->mode == RTFE_PE ? 2.0f : 1.0f) / (spbf > 2 ? spbf : 2);
      d.ds_cap = expect * 1.3f + 2 <= 15 ? 15 : (expect * 1.3f + 2 <= 31 ? 31 : 63);
      if (const char *e = getenv("RTFE_DS_CAP")) { const int v = atoi(e); if (v >= 1 && v <= 63) d.ds_cap = v; }      // (tests: lists that run full)
      d.ds_slot = ((int)sizeof(DsHdr) + d.ds_cap * (int)sizeof(DsRec) + 15) & ~15;
      {  // sets per classification pass: three where a width carries three or more (one pass over the tile's margins instead of two: PE's default
         // sweep 26.5 -> 24.3 ms per 6.5e7 rows, bench C4 - its width 1.5 carries three distinct sets - 308 -> 280 ms) and two workgroups of 512
         // still fit a CU's 160 KB of LDS.  (With tiles of 512 rows three sets cost a workgroup per CU - three instead of four - and lost on C4.)
         int per[kMaxScreens] = {0, 0, 0, 0}, mx = 0;
         for (int u = 0; u < d.nuset; ++u) { const int sidx = d.parm[d.uset_rep[u]].screen; if (++per[sidx] > mx) mx = per[sidx]; }
         d.ds_up = mx >= 3 ? 3 : 2;
         if (d.ds_up == 3 && (size_t)ds_lds_layout(c->ntrks, d.halo_rows, d.ds_pad + kDsTile + kDsRight, 3).total + sizeof(DevCfg) + 1024 > 80 * 1024) d.ds_up = 2;
         if (const char *e = getenv("RTFE_DS_UP")) { const int v = atoi(e); if (v >= 1 && v <= 3) d.ds_up = v; } }
      d.ds_sfloor = (hfloor < 4.0f ? hfloor : 4.0f) / 4.0f / 2.0f;
      d.ds_lean = getenv("RTFE_DS_LEAN") ? atoi(getenv("RTFE_DS_LEAN")) != 0 : 1;
      d.ds_quiet_s = getenv("RTFE_DS_QUIET_S") ? (float)atof(getenv("RTFE_DS_QUIET_S")) : 0.6f;
      d.ds_band_hi = getenv("RTFE_DS_BAND_HI") ? (float)atof(getenv("RTFE_DS_BAND_HI")) : 1.25f;
      d.ds_band_lo = getenv("RTFE_DS_BAND_LO") ? (float)atof(getenv("RTFE_DS_BAND_LO")) : 1.0f / 3.0f;
      if ((int)ds_lds_layout(c->ntrks, d.halo_rows, d.ds_pad + kDsTile + kDsRight, d.ds_up).total + 64 > 150 * 1024) d.dense_path = 0;
      if ((d.ds_pad + kDsTile + kDsRight) / kStrip * c->ntrks > 8 * kDsThreads) d.dense_path = 0; }      // (k_dseg keeps a lane's strips of the stale-minimum map in eight registers)
   {
      const int nwalk = c->nparmsets * c->ntrks;
      int rc = (24 * 1024) / (nwalk * 24);
      d.rec_cap = rc > 64 ? 64 : (rc < 8 ? 8 : rc);
      // deferred detections per walker and tile (beyond that they are finished on the spot) - sized below, once the rest of
      // k_decode's LDS is known, so that one more workgroup fits a CU where a smaller buffer buys that
      if (const char *e = getenv("RTFE_REC_CAP")) { const int v = atoi(e); if (v >= 4 && v <= d.rec_cap) d.rec_cap = v; } }      // (experiments: LDS per k_decode workgroup)
   if (d.find_zeros) d.rec_cap = 8;                                   // (the zero-crossing walkers store their events at once)
   if (!d.find_zeros) {
      // k_decode is latency bound: workgroups per CU are what counts.  A smaller record buffer is taken only if it lets one more workgroup reside.
      auto per_cu = [&](int rc) { DevCfg t = d; t.rec_cap = rc; return lds_wgs_per_cu((int)lds_layout(t).total + 64, 5500, INT_MAX); };      // (static LDS ~ 4 KB, allocation granularity, margin)
      int best = d.rec_cap;
      for (int rc = d.rec_cap; rc >= 8; --rc) if (per_cu(rc) > per_cu(best)) best = rc;
      d.rec_cap = best; }
   h->lds_bytes = (int)lds_layout(d).total + 64;
   if (h->lds_bytes > 160 * 1024 - 2048) { delete h; return fail(-14, "configuration needs %d bytes of LDS", h->lds_bytes); }
   if (getenv("RTFE_VERBOSE")) {
      const LdsLayout Ld = lds_layout(d);
      fprintf(stderr, "rtfe: LDS k_decode %d (tile..bits %u, bits..ldpos %u, ldpos..heights %u, recs %u, walkers %u)\n", h->lds_bytes, Ld.bits, Ld.ldpos - Ld.bits,
              Ld.heights - Ld.ldpos, Ld.nrec - Ld.recs, Ld.fdiff - Ld.walkers);
      fprintf(stderr, "rtfe: peak path %d, k_sift LDS %d (halo %d/%d rows, slots %d bytes, %d vectors per thread)\n", d.peak_path, d.pk_lds, d.pk_hl, d.pk_hr, d.pk_slot, sf_nv(d));
      for (int sidx = 0; sidx < d.nscreens; ++sidx) fprintf(stderr, "rtfe: screen %d W %d rise_i %d minpk_i %d sure_i %d\n", sidx, d.screen[sidx].W, d.screen[sidx].rise_i, d.screen[sidx].minpk_i, d.screen[sidx].sure_i); }
   hipDeviceProp_t prop;
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { delete h; return fail(-20, "no HIP device"); }
   h->num_cus = prop.multiProcessorCount;
   if (hipMalloc(&h->d_dev, sizeof(DevCfg)) != hipSuccess) { delete h; return fail(-21, "hipMalloc failed"); }
   if (hipMemcpy(h->d_dev, &d, sizeof(DevCfg), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(h->d_dev); delete h; return fail(-22, "hipMemcpy failed"); }
   raise_dynamic_lds(reinterpret_cast<const void *>(k_decode), h->lds_bytes);
   h->zeros_kernel = getenv("RTFE_ZEROS_KERNEL") ? atoi(getenv("RTFE_ZEROS_KERNEL")) != 0 : 1;
   h->diffz_kernel = getenv("RTFE_DIFFZ_KERNEL") ? atoi(getenv("RTFE_DIFFZ_KERNEL")) != 0 : 1;
   if (!(d.find_zeros && d.differentiate) || d.mode == RTFE_WW) h->diffz_kernel = 0;      // (k_diffz covers every track count, -invert and every deskew delay)
   h->side = nullptr; h->overlap = getenv("RTFE_OVERLAP") ? atoi(getenv("RTFE_OVERLAP")) != 0 : 1;
   h->graphs = getenv("RTFE_GRAPHS") ? atoi(getenv("RTFE_GRAPHS")) != 0 : 0;
   memset(h->gcache, 0, sizeof h->gcache); h->gstamp = 0;
   h->bursts_wpr = getenv("RTFE_BURSTS_WPR") ? atoi(getenv("RTFE_BURSTS_WPR")) : 0;
   h->ds_order = getenv("RTFE_DS_ORDER") ? atoi(getenv("RTFE_DS_ORDER")) : 1;
   h->dchain_wgs = getenv("RTFE_DCHAIN_WGS") ? atoi(getenv("RTFE_DCHAIN_WGS")) : 16;
   h->prep_wgs = getenv("RTFE_PREP_WGS") ? atoi(getenv("RTFE_PREP_WGS")) : 32;
   h->prep_run = getenv("RTFE_PREP_RUN") ? atoi(getenv("RTFE_PREP_RUN")) : 8;
   if (h->prep_run < 1 || h->prep_run > kPrepMaxRun) h->prep_run = 8;
   h->work_cap = getenv("RTFE_WORK_CAP") ? atoll(getenv("RTFE_WORK_CAP")) : -1;
   h->ccap_max = getenv("RTFE_CCAP") ? atoll(getenv("RTFE_CCAP")) : 0;
   h->dense_stop = getenv("RTFE_DENSE_STOP") ? atoi(getenv("RTFE_DENSE_STOP")) : 99;
   h->dseg_wgs = getenv("RTFE_DSEG_WGS") ? atoi(getenv("RTFE_DSEG_WGS")) : 0;
   h->dseg_threads = getenv("RTFE_DSEG_THREADS") ? atoi(getenv("RTFE_DSEG_THREADS")) : 0;
   h->seg_cap = getenv("RTFE_SEG_CAP") ? atoll(getenv("RTFE_SEG_CAP")) : 0;
   h->peak_stop = getenv("RTFE_PEAK_STOP") ? atoi(getenv("RTFE_PEAK_STOP")) : 99;
   h->sift_wgs = getenv("RTFE_SIFT_WGS") ? atoi(getenv("RTFE_SIFT_WGS")) : 0;
   h->sift_generic = getenv("RTFE_SIFT_GENERIC") != nullptr;
   h->sift_per_screen = !(getenv("RTFE_SIFT_PER_SCREEN") && atoi(getenv("RTFE_SIFT_PER_SCREEN")) == 0);
   h->dseg_generic = getenv("RTFE_DSEG_GENERIC") != nullptr;
   // (k_zeros packs two tracks' 16-bit states into a lane and reads the rows where they lie: no -invert, no deskew delays, a threshold inside int16)
   if (d.invert || d.maxskew > 0 || d.ntrks < 2 || d.zc_peak_i < 1 || d.zc_peak_i > 32767 || !d.zc_parallel) h->zeros_kernel = 0;      // (RTFE_ZC_PARALLEL=0: k_decode's sequential walk, for the tests)
   if (d.peak_path) {                 // (wide rows - 16 tracks and more - do not fit k_sift's tile into LDS: peak_path is off then and the kernel is never launched)
      raise_dynamic_lds(reinterpret_cast<const void *>(sf_kernel(sf_wmax(d), sf_threads(d), sf_nv(d))), d.pk_lds);
      for (int sc = 0; sc < kMaxScreens; ++sc) h->sfs_occ[sc] = 0;
      if (sf_special(h)) for (int sc = 0; sc < d.nscreens; ++sc) {
         raise_dynamic_lds(reinterpret_cast<const void *>(sf_special_sc(h, sc)), sfs_lds_sc(d, sc));
         int nb = 0;
         if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(sf_special_sc(h, sc)), sfs_threads(d), (size_t)sfs_lds_sc(d, sc)) == hipSuccess && nb >= 1) h->sfs_occ[sc] = nb; } }
   if (d.dense_path) raise_dynamic_lds(reinterpret_cast<const void *>(ds_kernel(h)), (int)ds_lds_layout(d.ntrks, d.halo_rows, d.ds_pad + kDsTile + kDsRight, d.ds_up).total + 64);
   (void)hipGetLastError();          // (a refused attribute must not linger as the process' "last error": the caller's runtime would report it as its own)
   if (getenv("RTFE_VERBOSE") && d.peak_path) {
      int nb = -1;
      const sfs_kernel_t sfs = sf_special(h);
      const int thr = sfs ? sfs_threads(d) : sf_threads(d), lds = sfs ? sfs_lds(d) : d.pk_lds;
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, sfs ? reinterpret_cast<const void *>(sfs) : reinterpret_cast<const void *>(sf_kernel(sf_wmax(d), sf_threads(d), sf_nv(d))), thr, (size_t)lds);
      fprintf(stderr, "rtfe: k_sift%s %d threads, %d bytes of LDS: %d workgroups per CU (occupancy API), %d CUs\n", sfs ? "_s" : "", thr, lds, nb, h->num_cus); }
   *out = h;
   return 0; }

constexpr int kTimingRing = 64;
static_assert(kTimingRing <= 64, "rtfe_handle::ev_ran holds 64 sets");
static void timing_free(rtfe_handle *h) {
   if (!h->ev0) return;
   for (int r = 0; r < kTimingRing; ++r) for (int i = 0; i < kNumKernels; ++i) { (void)hipEventDestroy(h->ev0[r][i]); (void)hipEventDestroy(h->ev1[r][i]); }
   delete[] h->ev0; delete[] h->ev1; h->ev0 = nullptr; h->ev1 = nullptr; }

extern "C" int rtfe_set_timing(rtfe_handle *h, int enable) {
   if (!h) return fail(-1, "null argument");
   if (enable && !h->timing) {
      h->ev0 = new hipEvent_t[kTimingRing][12]; h->ev1 = new hipEvent_t[kTimingRing][12];
      for (int r = 0; r < kTimingRing; ++r) for (int i = 0; i < kNumKernels; ++i)
      {
         const bool ok0 = hipEventCreate(&h->ev0[r][i]) == hipSuccess;
         const bool ok1 = ok0 && hipEventCreate(&h->ev1[r][i]) == hipSuccess;
         if (!ok1) {
            // (no half-made ring left behind - the events made so far are destroyed with it, the lone ev0 of this slot too)
            if (ok0) (void)hipEventDestroy(h->ev0[r][i]);
            for (int r2 = 0; r2 <= r; ++r2) for (int i2 = 0; i2 < (r2 < r ? kNumKernels : i); ++i2) { (void)hipEventDestroy(h->ev0[r2][i2]); (void)hipEventDestroy(h->ev1[r2][i2]); }
            delete[] h->ev0; delete[] h->ev1; h->ev0 = nullptr; h->ev1 = nullptr;
            return fail(-40, "hipEventCreate failed"); } }
      h->ev_next = 0; h->ev_pending = 0; }
   if (!enable && h->timing) timing_free(h);
   h->timing = enable != 0;
   return 0; }

extern "C" int rtfe_kernel_ms(rtfe_handle *h, float *out) {
   if (!h || !out || !h->timing) return fail(-41, "timing is not enabled");
   const int n = h->ev_pending < kTimingRing ? h->ev_pending : kTimingRing;
   for (int i = 0; i < kNumKernels; ++i) out[i] = 0;
   for (int k = 0; k < n; ++k) {
      const int r = ((h->ev_next - 1 - k) % kTimingRing + kTimingRing) % kTimingRing;
      for (int i = 0; i < kNumKernels; ++i) {
         float ms = 0;
         if (hipEventSynchronize(h->ev1[r][i]) != hipSuccess) return fail(-42, "hipEventSynchronize failed");
         if (hipEventElapsedTime(&ms, h->ev0[r][i], h->ev1[r][i]) != hipSuccess) return fail(-43, "hipEventElapsedTime failed");
         if ((h->ev_ran[r] >> i) & 1u) out[i] += ms; } }
   h->ev_pending = 0;
   return n; }

extern "C" void rtfe_destroy(rtfe_handle *h) {
   if (!h) return;
   if (h->timing) timing_free(h);
   drop_graphs(h);
   if (h->side) { (void)hipEventDestroy(h->ev_fork); (void)hipEventDestroy(h->ev_join); (void)hipEventDestroy(h->ev_fork2); (void)hipEventDestroy(h->ev_join2); (void)hipStreamDestroy(h->side); }
   (void)hipFree(h->d_dev);
   delete h; }

extern "C" int rtfe_pkww_width(const rtfe_handle *h, int parmset) {
   return (h && parmset >= 0 && parmset < h->dev.nparm) ? h->dev.parm[parmset].W : -1; }

constexpr int kBrRoundsMax = 1024;                                  // k_bursts_cnt / _emit: a workgroup per round of the zone search, at most this many (else one workgroup does them all)

extern "C" int64_t rtfe_max_bursts(const rtfe_handle *h, int64_t nrows) {
   return (nrows / kChunkRows) / h->dev.gap_chunks + 4; }

// ---- the workspace of a scan: every region's offset and every capacity that depends on the row count, worked out once, in the regions' order:
//   scratch | quiet words | rounds' counts | burst control | dir | chain | pool | hard | ovf | qtile | tstart | crec | eref | extra | cst | segs | gfire | dead | slot | total
// (dir .. gfire: the peak path's; dead, slot: the dense path's - a region of a path the handle does not take has no bytes.  From the control blocks on every region
//  starts on a multiple of 256 bytes.)
struct WsLayout {
   long long nwords, max_bursts, ptiles, dtiles;      // 64-bit words of the quiet map; bursts the table holds; tiles of k_sift (kSfTile rows) and of k_dseg (kDsTile rows)
   long long ccap, seg_cap, work_cap; int hard_cap;   // records of a stream; segments; places of k_prep's work list; deferred candidates
   size_t scratch, qwords, rtot, ctl, dir, chain, pool, hard, ovf, qtile, tstart, crec, eref, extra, cst, segs, gfire, work, dead, slot, total; };

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

static WsLayout ws_layout(const rtfe_handle *h, int64_t nrows) {
   const DevCfg &d = h->dev;
   const bool pk = d.peak_path != 0, ds = d.dense_path != 0;
   const size_t nlists = (size_t)d.nscreens * d.ntrks, nchains = (size_t)d.nparm * d.ntrks;
   WsLayout L;
   L.nwords = ((nrows / kChunkRows + 1) + 63) / 64 + 1;
   L.max_bursts = rtfe_max_bursts(h, nrows);
   L.ptiles = (nrows + kSfTile - 1) / kSfTile;
   L.dtiles = (nrows + kDsTile - 1) / kDsTile;
   // (a stream's capacity: every slot's worth of records and a marker per tile.  Deferred candidates add up to three records each; a stream
   //  that outgrows the capacity through them - its slots would have to be full of records without margins as well - is not built, and its
   //  chains give up.  RTFE_CCAP: a smaller one, for the tests)
   L.ccap = L.ptiles * (d.pk_slot / 8 + 1) + 64;
   if (h->ccap_max > 0 && h->ccap_max < L.ccap) L.ccap = h->ccap_max;
   // (two deferred candidates per tile and list: a clean NRZI tape defers 0.05 % of its candidates, a noisy parameter sweep with wide windows one or two per tile and list;
   //  past the capacity a candidate becomes a "minimum unknown" record, and the chain that gets there gives up.  k_sift_s: a wave takes the list's places a chunk at a time)
   const long long sift_wgs = L.ptiles < (long long)h->num_cus * 8 ? L.ptiles : (long long)h->num_cus * 8;
   const long long hard = L.ptiles * d.nscreens * d.ntrks * 2 + 4096 + sift_wgs * 4 * kSfHardChunk * d.nscreens;
   L.hard_cap = (int)(hard > 0x3fffffffll ? 0x3fffffffll : hard);
   L.seg_cap = 0;
   if (pk) L.seg_cap = h->seg_cap >= 1 ? h->seg_cap
                                       : (L.ccap / d.pk_seg_recs + 1) * d.nscreens * d.ntrks * (d.nparm < 2 ? 1 : 2) + L.max_bursts * d.nparm * d.ntrks + 64;
   // the regions in order: one that is `on` starts at the cursor and moves it to the next multiple of 256 bytes behind its end
   size_t off = 0;
   auto take = [&off](bool on, size_t bytes) { const size_t at = off; if (on) off = align256(off + bytes); return at; };
   L.scratch = 0;                                                                  // the BurstScratch block
   L.qwords = kScratchBytes;                                                       // the quiet map, a bit per 64 rows (not padded: the counts follow at once)
   L.rtot = L.qwords + (size_t)L.nwords * 8;                                       // the zone search's counts per round
   off = align256(L.rtot + (size_t)kBrRoundsMax * 4);
   L.ctl = take(true, (size_t)L.max_bursts * sizeof(BurstCtl));                    // burst control blocks
   L.dir = take(pk, (size_t)(L.ptiles + 1) * nlists * sizeof(PeakDir));            // directory of the tiles' lists
   L.chain = take(pk, (size_t)L.max_bursts * nchains * sizeof(float));             // per-chain baseline (k_gain -> k_emit)
   L.pool = take(pk, (size_t)L.ptiles * nlists * (size_t)d.pk_slot);               // record pool: one slot per (tile, screen, head)
   L.hard = take(pk, (size_t)L.hard_cap * sizeof(SfHard));                         // the candidates k_sift deferred (k_sift_hard)
   L.ovf = take(pk, (size_t)L.hard_cap * kSfOvfBytes);                             // their overflow slots
   L.qtile = take(pk, (size_t)L.ptiles * 2);                                       // the tiles' quiet bits (k_sift -> k_qpack)
   L.tstart = take(pk, ((size_t)L.ptiles + 2 * ((size_t)(L.ptiles + 1023) / 1024) + 2) * nlists * 4);      // the streams' tile offsets | chunk totals | chunk offsets | stream totals (k_pscan)
   L.crec = take(pk, (size_t)L.ccap * nlists * sizeof(CRec));                      // the streams (k_prep): 16-byte records
   L.eref = take(pk, (size_t)L.ccap * nlists * 8);                                 // a margin block per record, in stream order
   L.extra = take(pk, (size_t)L.ptiles * nlists * 4);                              // how many records a list's deferred candidates add to (or take from) its stream (k_sift_hard -> k_pscan)
   L.cst = take(pk, (size_t)L.max_bursts * nchains * sizeof(ChainSt));             // the chains between k_gain (heads), k_gain_s (steady stretches) and k_gain (tails)
   L.segs = take(pk, (size_t)L.seg_cap * sizeof(GsSeg));                           // the segments of the chains' steady stretches (k_segplan -> k_gain_seg -> k_gain_join)
   L.gfire = take(pk, (size_t)L.seg_cap * (size_t)(d.pk_seg_recs > 0 ? d.pk_seg_recs : 0) * 4);      // per record of a segment: the gain in force if it fired (k_gain_seg -> k_emit_seg)
   // k_prep's work list for k_clear lives in the gains' region - nothing reads it behind k_clear; 8 bytes a place, counted in an int
   // (RTFE_WORK_CAP, tests: a list that runs full - what does not fit stays unmarked, the general step's)
   L.work = L.gfire;
   L.work_cap = (long long)((off - L.gfire) / 8);
   if (h->work_cap >= 0 && h->work_cap < L.work_cap) L.work_cap = h->work_cap;
   if (L.work_cap > 0x7ffffe00ll) L.work_cap = 0x7ffffe00ll;
   L.dead = take(ds, (size_t)L.dtiles * d.nscreens);                               // the dense path: per (tile, width) "nothing above the screen"
   L.slot = take(ds, (size_t)L.dtiles * kDsJ * d.nuset * d.ntrks * (size_t)d.ds_slot + 256);      // the sub-segments' slots, the bands in their headers (+ a slot's worth: k_dchain reads nine 16-byte units of the last slot)
   L.total = off + 256;
   return L; }

extern "C" size_t rtfe_workspace_bytes(const rtfe_handle *h, int64_t nrows) { return ws_layout(h, nrows).total; }

extern "C" int64_t rtfe_event_capacity(const rtfe_handle *h, int64_t nrows) {
   const double per_track = (double)nrows * h->dev.cap_frac + 128.0 * (double)rtfe_max_bursts(h, nrows) + (double)kMarginRows;
   return (int64_t)(per_track * h->dev.nparm * h->dev.ntrks) + 4096; }

// the regions as the kernels take them
struct WsView {
   BurstScratch *scratch; unsigned long long *qwords; uint32_t *rtot; BurstCtl *ctl;
   PeakDir *dir; float *chain; unsigned char *pool; SfHard *hard; unsigned char *ovf; uint16_t *qtile;
   uint32_t *tstart, *ctotc, *coff, *ctot;      // the tstart region: tile offsets | chunk totals | chunk offsets | stream totals
   CRec *crec; uint2 *eref; int *extra; ChainSt *cst; GsSeg *segs; float *gfire; unsigned long long *work;
   unsigned char *dead, *slot; };

template <class T> static T *ws_at(void *ws, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(ws) + off); }

static WsView ws_view(const rtfe_handle *h, const WsLayout &L, void *ws) {
   WsView w;
   w.scratch = ws_at<BurstScratch>(ws, L.scratch); w.qwords = ws_at<unsigned long long>(ws, L.qwords); w.rtot = ws_at<uint32_t>(ws, L.rtot); w.ctl = ws_at<BurstCtl>(ws, L.ctl);
   w.dir = ws_at<PeakDir>(ws, L.dir); w.chain = ws_at<float>(ws, L.chain); w.pool = ws_at<unsigned char>(ws, L.pool); w.hard = ws_at<SfHard>(ws, L.hard);
   w.ovf = ws_at<unsigned char>(ws, L.ovf); w.qtile = ws_at<uint16_t>(ws, L.qtile);
   const size_t nlists = h->dev.peak_path ? (size_t)h->dev.nscreens * h->dev.ntrks : 0, nsc = (size_t)(L.ptiles + 1023) / 1024;      // chunks of 1024 tiles (k_pscan)
   w.tstart = ws_at<uint32_t>(ws, L.tstart); w.ctotc = w.tstart + (size_t)L.ptiles * nlists; w.coff = w.ctotc + nsc * nlists; w.ctot = w.coff + nsc * nlists;
   w.crec = ws_at<CRec>(ws, L.crec); w.eref = ws_at<uint2>(ws, L.eref); w.extra = ws_at<int>(ws, L.extra); w.cst = ws_at<ChainSt>(ws, L.cst);
   w.segs = ws_at<GsSeg>(ws, L.segs); w.gfire = ws_at<float>(ws, L.gfire); w.work = ws_at<unsigned long long>(ws, L.work);
   w.dead = ws_at<unsigned char>(ws, L.dead); w.slot = ws_at<unsigned char>(ws, L.slot);
   return w; }

static int launch_check(const char *what) {
   hipError_t e = hipGetLastError();
   if (e != hipSuccess) return fail(-30, "%s: %s", what, hipGetErrorString(e));
   return 0; }

// the handle's side stream (made at the first scan that wants it - outside any stream capture)
static void ensure_side(rtfe_handle *h) {
   if (h->side || !h->overlap) return;
   // (the side stream's kernels are a few workgroups each, the main stream's fill the chip: at the default priority k_bursts_tail sat behind k_prep's
   //  workgroups for 0.25 ms once k_sift_hard - fewer deferred candidates under the raised floor - no longer held k_prep back)
   int pr_least = 0, pr_greatest = 0;
   (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
   if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, pr_greatest) != hipSuccess) { (void)hipGetLastError(); h->side = nullptr; h->overlap = 0; }
   else { (void)hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming); (void)hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
          (void)hipEventCreateWithFlags(&h->ev_fork2, hipEventDisableTiming); (void)hipEventCreateWithFlags(&h->ev_join2, hipEventDisableTiming); } }

// rtfe_scan's arguments
struct ScanArgs {
   const int16_t *d_rows; int64_t nrows, own_rows, row_base; int first_is_tape_start;
   void *d_workspace; size_t workspace_bytes;
   rtfe_burst *d_bursts; int64_t max_bursts; int32_t *d_nbursts;
   uint32_t *d_counts; rtfe_event *d_events; int64_t event_capacity; void *stream; };

// what a captured graph of a scan is good for: every argument but the stream
static void graph_key(const ScanArgs &a, unsigned long long key[13]) {
   auto u = [](auto v) { return (unsigned long long)(uintptr_t)v; };
   const unsigned long long k[13] = {u(a.d_rows), u(a.nrows), u(a.own_rows), u(a.row_base), u(a.first_is_tape_start), u(a.d_workspace), u(a.workspace_bytes),
                                     u(a.d_bursts), u(a.max_bursts), u(a.d_nbursts), u(a.d_counts), u(a.d_events), u(a.event_capacity)};
   memcpy(key, k, sizeof k); }

// One scan's launches: what the three paths share, and the paths.
struct Scan {
   rtfe_handle *h; const DevCfg &d; const ScanArgs &a; hipStream_t st; WsLayout L; WsView w;
   long long nrows, row_base, nchunks, maxb;      // (nchunks: complete groups of 64 rows; maxb: bursts the caller's table and the workspace both hold)
   // every span's events are recorded by every scan (a span that does not run reads 0: rtfe_kernel_ms leaves it out, ev_ran)
   int evset; bool ran[kNumKernels];
   void t0s(int k, hipStream_t s) { ran[k] = true; if (h->timing) (void)hipEventRecord(h->ev0[evset][k], s); }
   void t1s(int k, hipStream_t s) { if (h->timing) (void)hipEventRecord(h->ev1[evset][k], s); }
   void t0(int k) { t0s(k, st); }
   void t1(int k) { t1s(k, st); }
   void skip_rest() {
      unsigned mask = 0;
      for (int k = 0; k < kNumKernels; ++k) if (ran[k]) mask |= 1u << k;
      if (h->timing) h->ev_ran[evset] = mask;
      for (int k = 0; k < kNumKernels; ++k) if (!ran[k]) { t0(k); t1(k); } }
   // quiet map -> burst table.  Long maps: a workgroup per round of 2^24 rows in two passes and a tail (k_bursts_cnt / _emit / _tail); short ones
   // (or absurdly long ones): the single workgroup that does the rounds in turn.  RTFE_BURSTS_WPR: words per round (tests: many rounds on a short tape).
   void launch_bursts(hipStream_t s) {
      const int wpr_env = h->bursts_wpr;
      const int wpr = (wpr_env >= 1 && wpr_env <= kBrWords) ? wpr_env : kBrWords;
      const long long rounds = (L.nwords + wpr - 1) / wpr;
      if ((wpr_env > 0 || rounds >= 3) && rounds <= kBrRoundsMax && d.debug != 5) {
         hipLaunchKernelGGL(k_bursts_cnt, dim3((unsigned)rounds), dim3(1024), 0, s, (const unsigned long long *)w.qwords, L.nwords, nchunks, wpr, d.gap_chunks, a.first_is_tape_start, maxb, w.rtot);
         hipLaunchKernelGGL(k_bursts_emit, dim3((unsigned)rounds), dim3(1024), 0, s, (const unsigned long long *)w.qwords, L.nwords, nchunks, nrows, wpr, d.gap_chunks, a.first_is_tape_start, a.d_bursts, maxb, (const uint32_t *)w.rtot);
         hipLaunchKernelGGL(k_bursts_tail, dim3(1), dim3(1024), 0, s, (int)rounds, (const uint32_t *)w.rtot, nrows, (long long)a.own_rows, d.ntrks, d.gap_chunks,
                            d.cap_frac, d.nparm, (long long)a.event_capacity, a.d_bursts, maxb, w.scratch, a.d_nbursts); }
      else
         hipLaunchKernelGGL(k_bursts, dim3(1), dim3(1024), 0, s, (const unsigned long long *)w.qwords, L.nwords, nchunks, nrows, (long long)a.own_rows, d.ntrks,
                            d.gap_chunks, a.first_is_tape_start, d.cap_frac, d.nparm, (long long)a.event_capacity, a.d_bursts, maxb, w.scratch, a.d_nbursts, d.debug == 5 ? 1 : 0); }
   // the restart rows of all bursts (rtfe_gain.hip)
   void launch_zones(hipStream_t s) {
      hipLaunchKernelGGL(k_zones, dim3(h->num_cus * 8), dim3(64), 0, s, h->d_dev, a.d_rows, nrows, (const rtfe_burst *)a.d_bursts, (const BurstScratch *)w.scratch, w.ctl);
      if (d.invert)      // (an inverted -32768 is +32768, wider than a record: bursts that hold one go to the sample path's literal walk)
         hipLaunchKernelGGL(k_rails, dim3(h->num_cus * 8), dim3(64), 0, s, h->d_dev, a.d_rows, nrows, (const rtfe_burst *)a.d_bursts, (const BurstScratch *)w.scratch, w.ctl); }
   // kDecodeAll: every burst in one pass over its samples; kDecodeRedo: the bursts the peak path's or the dense path's chains gave up
   void launch_decode(int mode) {
      const DecodePlan dp = decode_plan(h);
      t0(kTDecode);
      hipLaunchKernelGGL(k_decode, dim3(h->num_cus * dp.per_cu), dim3(dp.threads), h->lds_bytes, st, h->d_dev, a.d_rows, nrows,
                         row_base, a.d_bursts, w.scratch, a.d_counts, a.d_events, 0xffffffffu, 0, 0, mode, w.ctl);
      t1(kTDecode); }
   // k_sift: the quiet bits and the lists of every tile
   void launch_sift() {
      t0(kTSift);
      const sfs_kernel_t sfs = sf_special(h);
      const int pthreads = sfs ? sfs_threads(d) : sf_threads(d), plds = sfs ? sfs_lds(d) : d.pk_lds;
      int spc = lds_wgs_per_cu(plds, 512, 32 / (pthreads / 64));
      if (h->sift_wgs >= 1 && h->sift_wgs < spc) spc = h->sift_wgs;
      if (spc < 1) spc = 1;
      long long pgrid = (long long)h->num_cus * spc;
      if (pgrid > L.ptiles) pgrid = L.ptiles;
      if (sfs) {
         for (int sc = 0; sc < d.nscreens; ++sc) {
            SfArgs sa;
            sa.rows = a.d_rows; sa.nrows = nrows; sa.ntiles = (int)L.ptiles; sa.qtile = sc == 0 ? w.qtile : nullptr; sa.dir = w.dir; sa.pool = w.pool; sa.hard = w.hard; sa.hard_cap = L.hard_cap;
            sa.hard_count = &w.scratch->hard_count; sa.dbg = w.scratch->scr; sa.hcap = d.pk_slot; sa.wave_cap = d.pk_wave_cap; sa.invert = d.invert;
            sa.quiet_i = d.quiet_i; sa.cfg = h->d_dev; sa.hi_i = d.screen[sc].sure_i;
            sa.cut = d.cut; sa.debug = d.debug; sa.defer = 1; sa.nscreens = d.nscreens; sa.sc = sc;
            const int lds_sc = sfs_lds_sc(d, sc);
            int spc_sc = lds_wgs_per_cu(lds_sc, 512, spc);
            if (h->sfs_occ[sc] >= 1 && spc_sc > h->sfs_occ[sc]) spc_sc = h->sfs_occ[sc];      // (persistent workgroups: never more than are resident at once - the registers may allow fewer than the LDS)
            if (spc_sc < 1) spc_sc = 1;
            long long grid_sc = (long long)h->num_cus * spc_sc;
            if (grid_sc > L.ptiles) grid_sc = L.ptiles;
            hipLaunchKernelGGL(sf_special_sc(h, sc), dim3((unsigned)grid_sc), dim3(pthreads), lds_sc, st, sa); } }
      else {
         const sf_kernel_t sfk = sf_kernel(sf_wmax(d), pthreads, sf_nv(d));
         hipLaunchKernelGGL(sfk, dim3((unsigned)pgrid), dim3(pthreads), d.pk_lds, st, (const DevCfg *)h->d_dev, a.d_rows, nrows, L.ptiles,
                            w.qtile, w.dir, w.pool, w.hard, L.hard_cap, &w.scratch->hard_count, w.scratch->scr); }
      t1(kTSift); }
   // the lists -> one stream of 16-byte records per (screen, head): the deferred candidates resolved (k_sift_hard), the streams' tile
   // offsets (k_pscan), the records copied over with their absolute rows, volts and entry references (k_prep)
   void launch_streams() {
      t0(kTPrep);
      const int nlists = d.nscreens * d.ntrks;
      const int nsc = (int)((L.ptiles + 1023) / 1024);                    // chunks of 1024 tiles (k_pscan)
      hipLaunchKernelGGL(k_sift_hard, dim3(h->num_cus * 16), dim3(256), 0, st, (const DevCfg *)h->d_dev, a.d_rows, nrows, (const SfHard *)w.hard, L.hard_cap,
                         (const int *)&w.scratch->hard_count, w.ovf, w.extra, w.scratch->dbg2);
      hipLaunchKernelGGL(k_pscan1, dim3(nsc), dim3(1024), 0, st, (const PeakDir *)w.dir, (const int *)w.extra, (int)L.ptiles, nlists, w.tstart, w.ctotc);
      hipLaunchKernelGGL(k_pscan2, dim3(1), dim3(1024), 0, st, nsc, nlists, (const uint32_t *)w.ctotc, w.coff, w.ctot);
      PrepArgs ppa; ppa.nlists = nlists; ppa.ntrks = d.ntrks; ppa.hcap = d.pk_slot; ppa.run = h->prep_run; ppa.mv = d.maxvolts;
      // (workgroups per CU: 4 / 8 / 16 measured 0.51 / 0.47 / 0.42 ms for the span on C2 when half a wave took a list - the more lists in flight the better; a wave takes a
      //  run of prep_run tiles of one stream now, RTFE_PREP_RUN, and 32 has not been tuned again for that shape)
      hipLaunchKernelGGL(k_prep, dim3(h->num_cus * (h->prep_wgs >= 1 && h->prep_wgs <= 4096 ? h->prep_wgs : 32)), dim3(256), 0, st, ppa, (const PeakDir *)w.dir, (const unsigned char *)w.pool, (const unsigned char *)w.ovf,
                         (const uint32_t *)w.tstart, (const uint32_t *)w.coff, (const uint32_t *)w.ctot, L.ptiles, L.ccap, w.crec, w.eref, w.work, L.work_cap, &w.scratch->prep_work);
      hipLaunchKernelGGL(k_clear, dim3(h->num_cus * 4), dim3(256), 0, st, (const unsigned long long *)w.work, L.work_cap, (const int *)&w.scratch->prep_work, (const uint32_t *)w.ctot, L.ccap, w.crec);
#ifdef RTFE_CPU_EMUL
      if (getenv("RTFE_PREP_CHECK")) hipLaunchKernelGGL(k_prep_check, dim3(1), dim3(64), 0, st, (const DevCfg *)h->d_dev, (const uint32_t *)w.ctot, L.ccap, (const CRec *)w.crec);
      if (getenv("RTFE_PREP_CHECK") && atoi(getenv("RTFE_PREP_CHECK")) > 1)
         hipLaunchKernelGGL(k_prep_shapes, dim3(1), dim3(64), 0, st, nlists, (int)d.pk_slot, h->prep_run, L.ptiles, L.ccap, (const PeakDir *)w.dir, (const unsigned char *)w.pool, (const uint32_t *)w.ctot);
#endif
      t1(kTPrep); }
   // the chains: from the restart row until the baseline is fixed (k_gain, mode 0), the steady stretch (k_gain_s), whatever that stopped at (k_gain, mode 1)
   void launch_chains() {
      t0(kTGain);
      for (int mode = 0; mode < 2; ++mode) {
         if (mode == 1) t0(kTGainTail);
         hipLaunchKernelGGL(k_gain, dim3(h->num_cus * 4), dim3(64), 0, st, (const DevCfg *)h->d_dev, mode, w.cst, nrows, row_base, (const rtfe_burst *)a.d_bursts,
                            w.scratch, w.ctl, a.d_counts, a.d_events, w.chain, (const CRec *)w.crec, (const uint2 *)w.eref, (const uint32_t *)w.tstart, (const uint32_t *)w.coff, (const uint32_t *)w.ctot, L.ccap,
                            (const unsigned char *)w.pool, L.ptiles, w.segs, L.seg_cap, a.d_rows);
         if (mode == 0) {
            t1(kTGain); t0(kTGainS);
            // the steady stretches: in segments, every one on its own, joined where the states agree bit for bit (rtfe_gain.hip)
            hipLaunchKernelGGL(k_gain_seg, dim3(h->num_cus * 16), dim3(64), 0, st, (const DevCfg *)h->d_dev, (const ChainSt *)w.cst, w.scratch, (const CRec *)w.crec, L.ccap, w.segs, (const int *)&w.scratch->nsegs, L.seg_cap, w.gfire);
            hipLaunchKernelGGL(k_gain_join, dim3(h->num_cus * 2), dim3(64), 0, st, (const DevCfg *)h->d_dev, w.cst, (const rtfe_burst *)a.d_bursts, w.scratch, (const BurstCtl *)w.ctl, a.d_counts, w.chain, w.segs);
            t1(kTGainS); } }
#ifdef RTFE_CPU_EMUL
      if (getenv("RTFE_PREP_CHECK") && atoi(getenv("RTFE_PREP_CHECK")) > 1 && d.pk_seg_recs > 0)
         hipLaunchKernelGGL(k_seg_shapes, dim3(1), dim3(64), 0, st, (const DevCfg *)h->d_dev, (const ChainSt *)w.cst, (const BurstScratch *)w.scratch, (const CRec *)w.crec, L.ccap,
                            (const GsSeg *)w.segs, L.seg_cap, (const float *)w.gfire);
#endif
      t1(kTGainTail); }
   // the heads' and tails' noted events (k_emit: a wave per chain at a time - a chain's head and tail hold a few dozen) are finished on the side stream
   // beside the segments' events (k_emit_seg): disjoint parts of the event lists, both only need the chains
   void launch_emit(hipStream_t side) {
      t0(kTEmit);
      hipStream_t se = st;
      if (side != st) { se = side; (void)hipEventRecord(h->ev_fork2, st); (void)hipStreamWaitEvent(se, h->ev_fork2, 0); }
      hipLaunchKernelGGL(k_emit, dim3(h->num_cus * 32), dim3(64), 0, se, h->d_dev, (const rtfe_burst *)a.d_bursts, (const BurstScratch *)w.scratch, (const BurstCtl *)w.ctl, (const uint32_t *)a.d_counts, a.d_events,
                         (const float *)w.chain, (const CRec *)w.crec, (const uint2 *)w.eref, L.ccap, (const unsigned char *)w.pool, (const ChainSt *)w.cst, a.d_rows, nrows, (const GsSeg *)w.segs);
      if (se != st) (void)hipEventRecord(h->ev_join2, se);
      hipLaunchKernelGGL(k_emit_seg, dim3(h->num_cus * 16), dim3(256), 0, st, (const DevCfg *)h->d_dev, (const ChainSt *)w.cst, (const BurstCtl *)w.ctl, a.d_events, (const CRec *)w.crec, (const uint2 *)w.eref, L.ccap,
                         (const unsigned char *)w.pool, (const GsSeg *)w.segs, (const int *)&w.scratch->nsegs, L.seg_cap, (const float *)w.gfire, (int)(L.max_bursts * d.nparm * d.ntrks), a.d_rows, nrows);
      if (se != st) (void)hipStreamWaitEvent(st, h->ev_join2, 0);
      hipLaunchKernelGGL(k_publish, dim3(h->num_cus < 64 ? h->num_cus : 64), dim3(256), 0, st, h->d_dev, nrows, a.d_bursts, w.scratch, w.ctl);
      if (d.nuset < d.nparm)      // parameter sets the front end cannot tell apart were ONE chain: its events into the other sets' regions
         hipLaunchKernelGGL(k_dup_sets, dim3(h->num_cus * 8), dim3(256), 0, st, (const DevCfg *)h->d_dev, (const rtfe_burst *)a.d_bursts, (const BurstScratch *)w.scratch, (const BurstCtl *)w.ctl, a.d_counts, a.d_events);
      t1(kTEmit); }
   // ---- the peak path: k_sift (quiet map + records) -> k_bursts -> k_zones -> k_gain -> k_emit -> k_publish -> whatever the chains gave up ----
   void launch_peak_path() {
      const int stop_after = h->peak_stop;
      // the scratch block and the deferred candidates' counts cleared, and - a handle's first scan - the screen's floor estimated from the samples (k_scan_begin)
      uint4 *const extra16 = ws_at<uint4>(a.d_workspace, L.extra);      // (the whole region, in 16-byte units)
      hipLaunchKernelGGL(k_scan_begin, dim3(h->num_cus * 4), dim3(256), 0, st, h->d_dev, w.scratch, extra16, (long long)((L.cst - L.extra) / 16), a.d_rows, nrows);
      launch_sift();
      // Two things only need k_sift's output and not each other: (a) quiet map -> burst table -> restart rows (k_qpack, k_bursts, k_zones:
      // latency-bound, a workgroup or a wave per burst) and (b) the lists -> the streams (k_sift_hard, k_pscan, k_prep).  (a) runs on a
      // stream of the handle's own beside (b) and joins in front of the chains (RTFE_OVERLAP=0: in line; its span then is work, else the
      // time it shared the device).
      hipStream_t sa = st;
      if (h->overlap && stop_after >= 99) {
         ensure_side(h);
         if (h->side) { sa = h->side; (void)hipEventRecord(h->ev_fork, st); (void)hipStreamWaitEvent(sa, h->ev_fork, 0); } }
      t0s(kTBursts, sa);
      hipLaunchKernelGGL(k_qpack, dim3(h->num_cus < 64 ? h->num_cus : 64), dim3(256), 0, sa, (const uint16_t *)w.qtile, L.ptiles, w.qwords, L.nwords);
      launch_bursts(sa);
      if (stop_after >= 3) launch_zones(sa);
      t1s(kTBursts, sa);
      if (sa != st) (void)hipEventRecord(h->ev_join, sa);
      launch_streams();
      if (sa != st) (void)hipStreamWaitEvent(st, h->ev_join, 0);        // join: the chains need both
      if (stop_after < 3) return;
      launch_chains();
      if (stop_after < 4) return;
      launch_emit(sa);
      if (stop_after < 5) return;
      launch_decode(kDecodeRedo);
      if (d.adapt_floor) hipLaunchKernelGGL(k_adapt_floor, dim3(1), dim3(1), 0, st, h->d_dev, (const BurstScratch *)w.scratch); }      // (the NEXT scan's screen)
   // ---- the dense sample path, PE and GCR peak detection (rtfe_dense.hip): the dense pass first - it reads every row anyway, and leaves the quiet map's bits
   // as well (k_quiet folded in: one pass over the tape less); bursts and restart rows behind it, then a lane per chain, then whatever the chains gave up ----
   void launch_dense_path() {
      (void)hipMemsetAsync(w.scratch, 0, kScratchBytes, st);
      (void)hipMemsetAsync(w.qwords, 0, (size_t)L.nwords * 8, st);         // (a tile writes its own byte: the map's tail stays "not quiet")
      const int dlds = (int)ds_lds_layout(d.ntrks, d.halo_rows, d.ds_pad + kDsTile + kDsRight, d.ds_up).total + 64;
      int dpc = lds_wgs_per_cu(dlds, 1024, 8);
      if (h->dseg_wgs >= 1 && h->dseg_wgs < dpc) dpc = h->dseg_wgs;
      if (dpc < 1) dpc = 1;
      long long dg = (long long)h->num_cus * dpc;
      if (dg > L.dtiles) dg = L.dtiles;
      t0(kTDseg);
      // (threads: fewer waves that fill the rounds of the all-lane phases better - 448 / 384 / 320 threads for 9 tracks - are SLOWER: G1's k_dseg 84.8 / 92.1 / 93.8 ms
      //  against 78.3 with 512: the kernel lives on its resident waves, not on its lane-task count; RTFE_DSEG_THREADS for experiments)
      int dthreads = kDsThreads;
      if (h->dseg_threads >= 64 && h->dseg_threads <= kDsThreads) dthreads = h->dseg_threads / 64 * 64;
      unsigned char *const qbytes = ws_at<unsigned char>(a.d_workspace, L.qwords);      // (the quiet map as k_dseg writes it: a byte a tile)
      hipLaunchKernelGGL(ds_kernel(h), dim3((unsigned)dg), dim3(dthreads), dlds, st, (const DevCfg *)h->d_dev, a.d_rows, nrows, L.dtiles, w.dead, qbytes, w.slot, w.scratch->scr);
      t1(kTDseg);
      t0(kTBursts);
      launch_bursts(st);
      launch_zones(st);
      t1(kTBursts);
      if (h->dense_stop < 2) return;      // (debugging: 1 = stop behind k_dseg, 2 = behind k_dchain)
      t0(kTDchain);
      if (h->ds_order) hipLaunchKernelGGL(k_dorder, dim3(1), dim3(1024), 0, st, (const rtfe_burst *)a.d_bursts, (const BurstScratch *)w.scratch, w.ctl, nrows);
      // (LDS per wave decides how many chains run side by side - the kernel holds ~240 VGPRs, eight waves per CU: the literal rows' cache is a chunk and the
      //  widest window + 2, not the 88 rows the widest window the library accepts would need)
      int wmax = 1;
      for (int i = 0; i < d.nparm; ++i) if (d.parm[i].W > wmax) wmax = d.parm[i].W;
      const int dcache = wmax + 2 + kDcChunk < kDcCache ? ((wmax + 2 + kDcChunk + 7) & ~7) : kDcCache;
      hipLaunchKernelGGL(k_dchain, dim3(h->num_cus * (h->dchain_wgs >= 1 && h->dchain_wgs <= 64 ? h->dchain_wgs : 16)), dim3(64), (size_t)(d.ds_slot < 144 ? 144 : d.ds_slot) * 64 + (size_t)dcache * 64 * 2, st, (const DevCfg *)h->d_dev, a.d_rows, nrows, row_base, (const rtfe_burst *)a.d_bursts,
                         w.scratch, w.ctl, a.d_counts, a.d_events, (const unsigned char *)w.dead, (const unsigned char *)w.slot, L.dtiles, h->ds_order);
      hipLaunchKernelGGL(k_publish, dim3(h->num_cus < 64 ? h->num_cus : 64), dim3(256), 0, st, h->d_dev, nrows, a.d_bursts, w.scratch, w.ctl);
      t1(kTDchain);
      if (h->dense_stop < 3) return;
      launch_decode(kDecodeRedo); }
   // ---- the sample path: quiet map -> bursts -> every burst in one pass over its samples (-zeros: k_zeros; -zeros -differentiate: k_diffz; differentiated peaks,
   // density detection, PE / GCR with RTFE_DENSE_PATH=0: k_decode) ----
   void launch_sample_path() {
      (void)hipMemsetAsync(w.scratch, 0, kScratchBytes, st);
      const int grid = (int)(L.nwords < (long long)h->num_cus * 8 ? L.nwords : (long long)h->num_cus * 8);
      t0(kTQuiet);
      hipLaunchKernelGGL(k_quiet, dim3(grid), dim3(256), 0, st, a.d_rows, nrows, d.ntrks, d.quiet_i, w.qwords, L.nwords);
      t1(kTQuiet);
      t0(kTBursts);
      launch_bursts(st);
      t1(kTBursts);
      if (d.find_zeros && !d.differentiate && h->zeros_kernel) {          // -zeros: the lean kernel of its own (rtfe_zeros.hip)
         t0(kTZeros);
         hipLaunchKernelGGL(zeros_kernel(d.ntrks), dim3(h->num_cus * (RTFE_ZP_WPS * 256 / kZpThreads)), dim3(kZpThreads), 0, st,      // persistent workgroups, a burst at a time
                            (const DevCfg *)h->d_dev, a.d_rows, nrows, row_base, a.d_bursts, w.scratch, a.d_counts, a.d_events);
         t1(kTZeros); }
      else if (h->diffz_kernel) {                                        // -zeros -differentiate: the transducer kernel (rtfe_diffz.hip), in the k_zeros span
         t0(kTZeros);
         hipLaunchKernelGGL(k_diffz, dim3(h->num_cus * 6), dim3(kDzThreads), 0, st, (const DevCfg *)h->d_dev, a.d_rows, nrows, row_base, a.d_bursts, w.scratch, a.d_counts, a.d_events);
         t1(kTZeros); }
      else launch_decode(kDecodeAll); } };

static int scan_launch(rtfe_handle *h, const ScanArgs &a) {
   if (!h || !a.d_rows || !a.d_workspace || !a.d_bursts || !a.d_nbursts || !a.d_counts || !a.d_events) return fail(-1, "null argument");
   if (h->dev.mode == RTFE_WW) return fail(-44, "Whirlwind tapes have no independent bursts: use rtfe_ww_scan");
   if (((uintptr_t)a.d_rows & 15) != 0) return fail(-31, "d_rows must be 16-byte aligned");
   const WsLayout L = ws_layout(h, a.nrows);
   if (a.workspace_bytes < L.total) return fail(-32, "workspace too small");
   // the peak path addresses rows with 32 bits and a record's margin entries by a 32-bit index (2-byte units) into pool + overflow slots
   if (h->dev.peak_path && (a.nrows >= 0x7ff00000ll || (L.qtile - L.pool) / 2 >= 0xffffffffull))
      return fail(-36, "%lld rows are too many for one rtfe_scan on the peak path: scan the tape in fragments (own_rows)", (long long)a.nrows);
   if (a.nrows <= 0 || a.max_bursts < 1) return fail(-33, "nothing to scan");
   if (a.own_rows <= 0 || a.own_rows > a.nrows) return fail(-35, "own_rows must be in (0, nrows]");
   Scan s = {h, h->dev, a, (hipStream_t)a.stream, L, ws_view(h, L, a.d_workspace), a.nrows, a.row_base, a.nrows / kChunkRows,
             a.max_bursts < L.max_bursts ? a.max_bursts : L.max_bursts, h->timing ? h->ev_next : 0, {false}};
   if (h->timing) { h->ev_next = (h->ev_next + 1) % kTimingRing; ++h->ev_pending; }
   if (h->dev.peak_path) s.launch_peak_path();
   else if (h->dev.dense_path) s.launch_dense_path();
   else s.launch_sample_path();
   s.skip_rest();      // (also behind RTFE_PEAK_STOP / RTFE_DENSE_STOP: the spans that did not run)
   return launch_check("rtfe_scan"); }

extern "C" int rtfe_set_graphs(rtfe_handle *h, int enable) {
   if (!h) return fail(-1, "null argument");
   h->graphs = enable != 0;
   return 0; }

extern "C" int rtfe_scan(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t own_rows, int64_t row_base, int first_is_tape_start,
                         void *d_workspace, size_t workspace_bytes,
                         rtfe_burst *d_bursts, int64_t max_bursts, int32_t *d_nbursts,
                         uint32_t *d_counts, rtfe_event *d_events, int64_t event_capacity, void *stream) {
   const ScanArgs a = {d_rows, nrows, own_rows, row_base, first_is_tape_start, d_workspace, workspace_bytes, d_bursts, max_bursts, d_nbursts, d_counts, d_events, event_capacity, stream};
   // (per-kernel timing records events between the launches, the debug counters are read by tools between scans, the legacy default stream cannot be
   //  captured: those scans are launched directly)
   if (!h || !h->graphs || h->timing || h->dev.debug || !stream) return scan_launch(h, a);
   hipStream_t st = (hipStream_t)stream;
   unsigned long long key[13];
   graph_key(a, key);
   for (int i = 0; i < kGraphCache; ++i) {
      rtfe_handle::GraphEnt &e = h->gcache[i];
      if (e.exec && memcmp(e.key, key, sizeof key) == 0) {
         e.stamp = ++h->gstamp;
         if (hipGraphLaunch(e.exec, st) != hipSuccess) return fail(-30, "rtfe_scan: hipGraphLaunch: %s", hipGetErrorString(hipGetLastError()));
         return 0; } }
   int slot = 0;                                                       // an empty place, else the least recently used
   for (int i = 0; i < kGraphCache; ++i) {
      if (!h->gcache[i].exec) { slot = i; break; }
      if (h->gcache[i].stamp < h->gcache[slot].stamp) slot = i; }
   // a new set of arguments: its launches captured (nothing runs while they are), instantiated, launched - into the least recently used place
   ensure_side(h);
   if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError(); h->graphs = 0;
      return scan_launch(h, a); }
   const int rc = scan_launch(h, a);
   hipGraph_t g = nullptr;
   const hipError_t ec = hipStreamEndCapture(st, &g);
   if (rc != 0) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); return rc; }      // (an argument the scan refuses: nothing was enqueued, the message stands)
   hipGraphExec_t ex = nullptr;
   if (ec != hipSuccess || !g || hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
      // (a runtime that cannot capture this sequence: the scan is launched directly, now and from here on)
      if (g) (void)hipGraphDestroy(g);
      (void)hipGetLastError(); h->graphs = 0;
      return scan_launch(h, a); }
   (void)hipGraphDestroy(g);
   rtfe_handle::GraphEnt &e = h->gcache[slot];
   if (e.exec) (void)hipGraphExecDestroy(e.exec);
   memcpy(e.key, key, sizeof key); e.exec = ex; e.stamp = ++h->gstamp;
   if (hipGraphLaunch(ex, st) != hipSuccess) return fail(-30, "rtfe_scan: hipGraphLaunch: %s", hipGetErrorString(hipGetLastError()));
   return 0; }

// Synchronous (copies three words back): what the last rtfe_scan on this workspace did.
extern "C" int rtfe_pack_events(rtfe_handle *h, const rtfe_burst *d_bursts, const int32_t *d_nbursts, int64_t max_bursts, const uint32_t *d_counts,
                                const rtfe_event *d_events, rtfe_event *d_packed, uint64_t packed_capacity, rtfe_pack_entry *d_plan, void *stream) {
   if (!h || !d_bursts || !d_nbursts || !d_counts || !d_events || !d_packed || !d_plan || max_bursts < 1) return fail(-2, "rtfe_pack_events: null argument");
   hipStream_t st = (hipStream_t)stream;
   const int lists = h->cfg.nparmsets * h->cfg.ntrks;
   hipLaunchKernelGGL(k_pack_plan, dim3(1), dim3(1024), 0, st, d_bursts, d_nbursts, (long long)max_bursts, d_counts, lists, d_plan);
   hipLaunchKernelGGL(k_pack_copy, dim3((unsigned)(h->num_cus * 8)), dim3(256), 0, st, d_bursts, d_nbursts, (long long)max_bursts, d_counts, lists, (const rtfe_pack_entry *)d_plan,
                      reinterpret_cast<const uint4 *>(d_events), reinterpret_cast<uint4 *>(d_packed), (unsigned long long)packed_capacity);
   const hipError_t e = hipGetLastError();
   if (e != hipSuccess) return fail(-30, "rtfe_pack_events: %s", hipGetErrorString(e));
   return 0; }

extern "C" int rtfe_find_end_mark(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t *d_first, void *stream) {
   if (!h || !d_rows || !d_first || nrows < 0) return fail(-2, "rtfe_find_end_mark: bad argument");
   hipStream_t st = (hipStream_t)stream;
   hipLaunchKernelGGL(k_end_mark_init, dim3(1), dim3(1), 0, st, reinterpret_cast<long long *>(d_first));
   if (nrows > 0) {
      long long blocks = (nrows + 255) / 256;
      if (blocks > (long long)h->num_cus * 16) blocks = (long long)h->num_cus * 16;
      hipLaunchKernelGGL(k_end_mark, dim3((unsigned)blocks), dim3(256), 0, st, d_rows, (long long)nrows, h->cfg.ntrks, reinterpret_cast<long long *>(d_first)); }
   const hipError_t e = hipGetLastError();
   if (e != hipSuccess) return fail(-30, "rtfe_find_end_mark: %s", hipGetErrorString(e));
   return 0; }

extern "C" int64_t rtfe_decimate_span_rows(int ntrks) { return ntrks >= 1 && ntrks <= RTFE_MAXTRKS ? dec_span_rows(ntrks) : 0; }

extern "C" int rtfe_decimate_rows(const int16_t *d_in, int64_t nrows_in, int ntrks, int64_t first, int64_t step, int16_t *d_out, int64_t out_cap_rows,
                                  int64_t *d_first_mark, void *stream) {
   if (!d_in || !d_out || !d_first_mark) return fail(-1, "rtfe_decimate_rows: null argument");
   if (ntrks < 1 || ntrks > RTFE_MAXTRKS) return fail(-3, "rtfe_decimate_rows: ntrks %d out of range", ntrks);
   if (step < 1 || first < 0 || nrows_in < 0) return fail(-34, "rtfe_decimate_rows: bad row range (nrows_in %lld, first %lld, step %lld)", (long long)nrows_in, (long long)first, (long long)step);
   if ((((uintptr_t)d_in | (uintptr_t)d_out) & 15) != 0) return fail(-31, "rtfe_decimate_rows: d_in and d_out must be 16-byte aligned");
   const int span = dec_span_rows(ntrks);
   const long long nwg = (nrows_in + span - 1) / span;
   if (nwg > 0x7fffffffll) return fail(-34, "rtfe_decimate_rows: %lld rows are more than a launch takes", (long long)nrows_in);
   if (step > nrows_in) step = nrows_in > 0 ? nrows_in : 1;          // (the same rows: out row 0 only, if any - and no sum below leaves 64 bits)
   const long long nkept = first < nrows_in ? (nrows_in - first + step - 1) / step : 0;
   if (out_cap_rows < nkept) return fail(-32, "rtfe_decimate_rows: %lld rows to write, room for %lld", nkept, (long long)out_cap_rows);
   const uintptr_t rb = 2 * (uintptr_t)ntrks, i0 = (uintptr_t)d_in, i1 = i0 + (uintptr_t)nrows_in * rb, o0 = (uintptr_t)d_out, o1 = o0 + (uintptr_t)nkept * rb;
   if (i0 < o1 && o0 < i1) return fail(-37, "rtfe_decimate_rows: d_in and d_out overlap (in place is not supported)");
   hipStream_t st = (hipStream_t)stream;
   hipLaunchKernelGGL(k_end_mark_init, dim3(1), dim3(1), 0, st, reinterpret_cast<long long *>(d_first_mark));
   if (nwg > 0)
      hipLaunchKernelGGL(k_decimate, dim3((unsigned)nwg), dim3(kDecWave), 0, st, d_in, (long long)nrows_in, ntrks, (long long)first, (long long)step, span, d_out,
                         reinterpret_cast<long long *>(d_first_mark));
   return launch_check("rtfe_decimate_rows"); }

extern "C" int rtfe_reset_floor(rtfe_handle *h, void *stream) {
   if (!h) return fail(-1, "null argument");
   hipLaunchKernelGGL(k_reset_floor, dim3(1), dim3(1), 0, (hipStream_t)stream, h->d_dev);
   return launch_check("rtfe_reset_floor"); }

extern "C" int rtfe_scan_stats(rtfe_handle *h, const void *d_workspace, int64_t *out) {
   if (!h || !d_workspace || !out) return fail(-1, "null argument");
   BurstScratch sc;
   if (hipMemcpy(&sc, d_workspace, sizeof sc, hipMemcpyDeviceToHost) != hipSuccess) return fail(-44, "hipMemcpy failed");
   out[0] = sc.nbursts; out[1] = sc.seg_failed; out[2] = (int64_t)sc.scr[3]; out[3] = (int64_t)sc.dbg[0]; out[4] = (int64_t)sc.dbg[1];
   for (int i = 0; i < 8; ++i) out[5 + i] = (int64_t)sc.why[i];
   out[21] = (int64_t)sc.min_height_key;      // 0x7fffffff - float bits of the smallest learned v_avg_height, 0: none (the Python binding turns it back)
   {  float fl = 0;                                // the floor the handle's NEXT scan screens against (k_adapt_floor has moved it behind this one), as float bits
      if (hipMemcpy(&fl, &h->d_dev->floor_now, sizeof fl, hipMemcpyDeviceToHost) != hipSuccess) return fail(-44, "hipMemcpy failed");
      uint32_t fb; memcpy(&fb, &fl, 4); out[22] = (int64_t)fb;
      memcpy(&fb, &sc.floor_used, 4); out[23] = (int64_t)fb; }      // the floor this scan's screen was built for
   for (int i = 0; i < 8; ++i) out[13 + i] = (int64_t)((h->dev.debug == 4 || h->dev.debug == 6 || h->dev.debug == 8 || h->dev.debug == 9) ? sc.dbg2[i] : sc.scr[i]);      // (RTFE_DEBUG=4: k_gain's cycle counters instead)      // RTFE_DEBUG=3: k_sift cycles per phase (copy, dense, owners, record bytes, hard candidates, rounds, rounds with one, tiles)
   return 0; }

extern "C" int rtfe_scan_exact(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t row_base,
                               int64_t reset_row, int64_t end_row, uint32_t parmset_mask, int screen_off,
                               void *d_workspace, size_t workspace_bytes,
                               rtfe_burst *d_burst, uint32_t *d_counts, rtfe_event *d_events, int64_t event_capacity,
                               void *stream) {
   if (!h || !d_rows || !d_workspace || !d_burst || !d_counts || !d_events) return fail(-1, "null argument");
   if (((uintptr_t)d_rows & 15) != 0) return fail(-31, "d_rows must be 16-byte aligned");
   if (workspace_bytes < kScratchBytes) return fail(-32, "workspace too small");
   if (reset_row < 0 || reset_row >= nrows || end_row <= reset_row) return fail(-34, "bad row range");
   if (end_row > nrows) end_row = nrows;
   hipStream_t st = (hipStream_t)stream;
   BurstScratch *scratch = reinterpret_cast<BurstScratch *>(d_workspace);
   const unsigned long long cap = (unsigned long long)(event_capacity / ((int64_t)h->dev.nparm * h->dev.ntrks));
   hipLaunchKernelGGL(k_setup_exact, dim3(1), dim3(1), 0, st, d_burst, scratch, (long long)reset_row, (long long)end_row,
                      cap > 0xffffffffull ? 0xffffffffull : cap);
   hipLaunchKernelGGL(k_decode, dim3(1), dim3(decode_plan(h).walker_threads), h->lds_bytes, st, h->d_dev, d_rows, (long long)nrows,
                      (long long)row_base, d_burst, scratch, d_counts, d_events, parmset_mask, screen_off, 1, (int)kDecodeAll, (BurstCtl *)nullptr);
   return launch_check("rtfe_scan_exact"); }

// ---- Whirlwind (include/rt_frontend.h) ----
extern "C" void rtfe_ww_initial_state(rtfe_ww_track *tracks, int ntrks) {
   memset(tracks, 0, sizeof(rtfe_ww_track) * (size_t)ntrks);
   for (int t = 0; t < ntrks; ++t) { tracks[t].agc_gain = 1.0f; tracks[t].v_avg_height = 4.0f; } }

extern "C" int rtfe_ww_scan(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t row_base, int64_t first_row, int64_t nscan, int64_t seed_row0,
                            const rtfe_ww_track *d_state_in, rtfe_ww_track *d_state_out, uint32_t *d_counts, rtfe_event *d_events, int64_t event_capacity,
                            uint32_t *d_flags, void *stream) {
   if (!h || !d_rows || !d_state_in || !d_state_out || !d_counts || !d_events || !d_flags) return fail(-1, "null argument");
   if (h->dev.mode != RTFE_WW) return fail(-40, "rtfe_ww_scan: the handle was not made for mode RTFE_WW");
   if (h->dev.find_zeros || h->dev.differentiate) return fail(-41, "rtfe_ww_scan: peak detection on the undifferentiated signal; this handle was made with -zeros / -differentiate (rtfe_ww_detector_scan)");
   if (h->dev.maxskew > 0 || h->dev.nparm != 1) return fail(-41, "rtfe_ww_scan: peak detection, one parameter set, deskew delays in the state (not in the configuration)");
   if (h->dev.parm[0].W > kWwRing) return fail(-42, "window wider than the state's ring");
   if (first_row < 0 || nscan <= 0 || first_row >= nrows || seed_row0 > first_row || event_capacity < 1) return fail(-43, "bad row range");
   hipLaunchKernelGGL(k_ww, dim3(1), dim3(64), 0, (hipStream_t)stream, (const DevCfg *)h->d_dev, d_rows, (long long)nrows, (long long)row_base,
                      (long long)first_row, (long long)nscan, (long long)seed_row0, d_state_in, d_state_out, d_counts, d_events, (long long)event_capacity, d_flags);
   return launch_check("rtfe_ww_scan"); }

// ---- Whirlwind with -zeros and / or -differentiate (include/rt_frontend.h) ----
static int ww_kind(const rtfe_handle *h) {
   if (!h || h->dev.mode != RTFE_WW) return -1;
   return h->dev.find_zeros ? (h->dev.differentiate ? RTFE_WW_DIFFZEROS : RTFE_WW_ZEROS) : (h->dev.differentiate ? RTFE_WW_DIFFPEAKS : RTFE_WW_PEAKS); }

extern "C" int rtfe_ww_state_kind(const rtfe_handle *h) { return ww_kind(h); }
// the path rtfe_scan takes for this handle, as rtfe_create decided it behind the environment knobs (scan_launch's branches in their order)
extern "C" int rtfe_detector_path(const rtfe_handle *h) {
   if (!h) return -1;
   if (h->dev.mode == RTFE_WW) return RTFE_PATH_WW;
   if (h->dev.peak_path) return RTFE_PATH_PEAK;
   if (h->dev.find_zeros && !h->dev.differentiate && h->zeros_kernel) return RTFE_PATH_ZEROS;
   if (h->diffz_kernel) return RTFE_PATH_DIFFZEROS;
   if (h->dev.dense_path) return RTFE_PATH_DENSE;
   return RTFE_PATH_SAMPLE; }

extern "C" size_t rtfe_ww_state_bytes(const rtfe_handle *h) {
   const int k = ww_kind(h);
   return k < 0 ? 0 : (k == RTFE_WW_PEAKS ? sizeof(rtfe_ww_track) : sizeof(rtfe_ww_dtrack)); }

extern "C" int rtfe_ww_detector_initial_state(const rtfe_handle *h, void *tracks, size_t state_bytes) {
   if (!h || !tracks) return fail(-1, "null argument");
   const int k = ww_kind(h);
   if (k < 0) return fail(-40, "rtfe_ww_detector_initial_state: the handle was not made for mode RTFE_WW");
   const size_t want = rtfe_ww_state_bytes(h) * (size_t)h->dev.ntrks;
   if (state_bytes != want) return fail(-45, "rtfe_ww_detector_initial_state: a state of %zu bytes, this handle's is %zu (%d tracks of %zu)", state_bytes, want, h->dev.ntrks, rtfe_ww_state_bytes(h));
   if (k == RTFE_WW_PEAKS) { rtfe_ww_initial_state((rtfe_ww_track *)tracks, h->dev.ntrks); return 0; }
   rtfe_ww_dtrack *st = (rtfe_ww_dtrack *)tracks;
   memset(st, 0, want);                                               // src/decoder.c:437: everything but what follows
   for (int t = 0; t < h->dev.ntrks; ++t) { st[t].kind = k; st[t].agc_gain = 1.0f; st[t].v_avg_height = 4.0f; }
   return 0; }

extern "C" int rtfe_ww_detector_scan(rtfe_handle *h, const int16_t *d_rows, int64_t nrows, int64_t row_base, int64_t first_row, int64_t nscan, int64_t seed_row0,
                                     const void *d_state_in, void *d_state_out, size_t state_bytes, uint32_t *d_counts, rtfe_ww_event *d_events,
                                     int64_t event_capacity, uint32_t *d_flags, void *stream) {
   if (!h || !d_rows || !d_state_in || !d_state_out || !d_counts || !d_events || !d_flags) return fail(-1, "null argument");
   const int k = ww_kind(h);
   if (k < 0) return fail(-40, "rtfe_ww_detector_scan: the handle was not made for mode RTFE_WW");
   if (k == RTFE_WW_PEAKS) return fail(-41, "rtfe_ww_detector_scan: this handle detects peaks on the undifferentiated signal (rtfe_ww_scan, rtfe_ww_track)");
   if (h->dev.maxskew > 0 || h->dev.nparm != 1) return fail(-41, "rtfe_ww_detector_scan: one parameter set, deskew delays in the state (not in the configuration)");
   const size_t want = sizeof(rtfe_ww_dtrack) * (size_t)h->dev.ntrks;
   if (state_bytes != want) return fail(-45, "rtfe_ww_detector_scan: a state of %zu bytes, this handle's is %zu (%d tracks of %zu: rtfe_ww_dtrack)", state_bytes, want, h->dev.ntrks, sizeof(rtfe_ww_dtrack));
   if (k == RTFE_WW_DIFFPEAKS && h->dev.parm[0].W > kWwRing) return fail(-42, "window wider than the state's ring");
   if (first_row < 0 || nscan <= 0 || first_row >= nrows || seed_row0 > first_row || event_capacity < 1) return fail(-43, "bad row range");
   hipLaunchKernelGGL(k_ww_det, dim3(1), dim3(64), 0, (hipStream_t)stream, (const DevCfg *)h->d_dev, d_rows, (long long)nrows, (long long)row_base,
                      (long long)first_row, (long long)nscan, (long long)seed_row0, k, (const rtfe_ww_dtrack *)d_state_in, (rtfe_ww_dtrack *)d_state_out,
                      d_counts, d_events, (long long)event_capacity, d_flags);
   return launch_check("rtfe_ww_detector_scan"); }

// ---- CSV text -> int16 rows on the device (include/rt_frontend.h; kernels in rtfe_csv.hip) ----
static uint32_t csv_blocks(uint64_t nbytes) { return (uint32_t)((nbytes + kCsvBlockBytes - 1) / kCsvBlockBytes); }
extern "C" size_t rtfe_csv_index_scratch_bytes(uint64_t nbytes) { return (size_t)csv_blocks(nbytes) * 8 + 16; }

extern "C" int rtfe_csv_index(const void *d_text, uint64_t nbytes, int is_last, uint32_t *d_starts, int64_t starts_cap, void *d_scratch, size_t scratch_bytes,
                              rtfe_csv_window *d_out, void *stream) {
   if (!d_text || !d_starts || !d_scratch || !d_out) return fail(-1, "rtfe_csv_index: null argument");
   if (((uintptr_t)d_text & 15) != 0) return fail(-31, "rtfe_csv_index: d_text must be 16-byte aligned");
   if (nbytes >= (1ull << 32)) return fail(-35, "rtfe_csv_index: a window of %llu bytes (shorter than 2^32)", (unsigned long long)nbytes);
   if (starts_cap < 0) return fail(-34, "rtfe_csv_index: starts_cap %lld", (long long)starts_cap);
   if (scratch_bytes < rtfe_csv_index_scratch_bytes(nbytes)) return fail(-32, "rtfe_csv_index: scratch too small");
   hipStream_t st = (hipStream_t)stream;
   const uint32_t nb = csv_blocks(nbytes);
   uint32_t *cnt = reinterpret_cast<uint32_t *>(d_scratch), *last = cnt + nb;
   const uint4 *text = reinterpret_cast<const uint4 *>(d_text);
   if (nb) hipLaunchKernelGGL(k_csv_count, dim3(nb), dim3(256), 0, st, text, (uint32_t)nbytes, cnt, last);
   hipLaunchKernelGGL(k_csv_scan, dim3(1), dim3(kCsvScanThreads), 0, st, nb, (uint32_t)nbytes, is_last != 0, cnt, last, d_starts, (long long)starts_cap, d_out);
   if (nb) hipLaunchKernelGGL(k_csv_starts, dim3(nb), dim3(256), 0, st, text, (uint32_t)nbytes, (const uint32_t *)cnt, (const uint32_t *)last, d_starts, (long long)starts_cap, d_out);
   return launch_check("rtfe_csv_index"); }

extern "C" int rtfe_csv_peak(const void *d_text, const uint32_t *d_starts, int64_t first_line, int64_t nlines, int ntrks, float scale, float *d_peak, void *stream) {
   if (!d_text || !d_starts || !d_peak) return fail(-1, "rtfe_csv_peak: null argument");
   if (ntrks < 1 || ntrks > RTFE_MAXTRKS) return fail(-3, "rtfe_csv_peak: ntrks %d out of range", ntrks);
   if (((uintptr_t)d_text & 15) != 0) return fail(-31, "rtfe_csv_peak: d_text must be 16-byte aligned");
   if (first_line < 0 || nlines < 0 || first_line + nlines >= (1ll << 32)) return fail(-34, "rtfe_csv_peak: bad line range");
   if (nlines == 0) return 0;
   hipLaunchKernelGGL(k_csv_peak, dim3((unsigned)((nlines + kCsvWaveLines - 1) / kCsvWaveLines)), dim3(kCsvWaveLines), 0, (hipStream_t)stream,
                      reinterpret_cast<const unsigned char *>(d_text), d_starts, (long long)first_line, (long long)nlines, ntrks, scale, d_peak);
   return launch_check("rtfe_csv_peak"); }

extern "C" int rtfe_csv_parse(const void *d_text, const uint32_t *d_starts, int64_t first_line, int64_t step, int64_t nkept, int ntrks, const int *perm, int invert,
                              float scale, float maxvolts, int16_t *d_rows, int64_t *d_clipped, void *stream) {
   if (!d_text || !d_starts || !d_rows || !d_clipped) return fail(-1, "rtfe_csv_parse: null argument");
   if (ntrks < 1 || ntrks > RTFE_MAXTRKS) return fail(-3, "rtfe_csv_parse: ntrks %d out of range", ntrks);
   if (perm) for (int k = 0; k < ntrks; ++k) if (perm[k] < 0 || perm[k] >= ntrks) return fail(-4, "rtfe_csv_parse: perm[%d] = %d out of range", k, perm[k]);
   if (((uintptr_t)d_text & 15) != 0) return fail(-31, "rtfe_csv_parse: d_text must be 16-byte aligned");
   if (first_line < 0 || step < 1 || nkept < 0 || first_line + (nkept ? (nkept - 1) * step + 1 : 0) >= (1ll << 32)) return fail(-34, "rtfe_csv_parse: bad line range");
   if (nkept == 0) return 0;
   CsvParseArgs a;
   a.text = reinterpret_cast<const unsigned char *>(d_text); a.starts = d_starts;
   a.first_line = first_line; a.step = step; a.nkept = nkept;
   a.ntrks = ntrks; a.invert = invert != 0; a.scale = scale; a.maxvolts = maxvolts;
   a.perm_lo = 0; a.perm_hi = 0;
   for (int k = 0; k < ntrks; ++k) {
      const unsigned long long c = (unsigned long long)(perm ? perm[k] : k);
      if (k < 12) a.perm_lo |= c << (5 * k); else a.perm_hi |= c << (5 * (k - 12)); }
   a.rows = d_rows; a.clipped = reinterpret_cast<unsigned long long *>(d_clipped);
   hipLaunchKernelGGL(k_csv_parse, dim3((unsigned)((nkept + kCsvWaveLines - 1) / kCsvWaveLines)), dim3(kCsvWaveLines), 0, (hipStream_t)stream, a);
   return launch_check("rtfe_csv_parse"); }

extern "C" int rtfe_csv_graph(const void *d_text, const uint32_t *d_starts, int64_t first_line, int64_t step, int64_t nkept, int ntrks, float scale,
                              int64_t first_sample, int64_t graphbin, float *d_bins, int64_t nbins, float *d_peak, void *stream) {
   if (!d_text || !d_starts || (!d_bins && nbins > 0)) return fail(-1, "rtfe_csv_graph: null argument");
   if (ntrks < 1 || ntrks > RTFE_MAXTRKS) return fail(-3, "rtfe_csv_graph: ntrks %d out of range", ntrks);
   if (((uintptr_t)d_text & 15) != 0) return fail(-31, "rtfe_csv_graph: d_text must be 16-byte aligned");
   if (first_line < 0 || step < 1 || nkept < 0 || first_line + (nkept ? (nkept - 1) * step + 1 : 0) >= (1ll << 32)) return fail(-34, "rtfe_csv_graph: bad line range");
   if (graphbin < 1) return fail(-34, "rtfe_csv_graph: graphbin %lld (samples per bin: at least 1)", (long long)graphbin);
   if (nbins < 0) return fail(-34, "rtfe_csv_graph: nbins %lld", (long long)nbins);
   if (first_sample < 0 || first_sample >= (1ll << 62)) return fail(-34, "rtfe_csv_graph: first_sample %lld", (long long)first_sample);
   if (nkept == 0 || (nbins == 0 && !d_peak)) return 0;
   CsvGraphArgs a;
   a.text = reinterpret_cast<const unsigned char *>(d_text); a.starts = d_starts;
   a.first_line = first_line; a.step = step; a.nkept = nkept;
   a.ntrks = ntrks; a.scale = scale;
   a.first_sample = first_sample; a.graphbin = graphbin; a.nbins = nbins;
   a.bins = reinterpret_cast<int *>(d_bins); a.peak = reinterpret_cast<int *>(d_peak);
   hipLaunchKernelGGL(k_csv_graph, dim3((unsigned)((nkept + kCsvWaveLines - 1) / kCsvWaveLines)), dim3(kCsvWaveLines), 0, (hipStream_t)stream, a);
   return launch_check("rtfe_csv_graph"); }

// ---- int16 rows -> CSV text on the device (include/rt_frontend.h; kernels in rtfe_csvout.hip) ----
// what the arguments admit: a refusal (negative), or whether every line of the window provably has the uniform length
static int co_plan(const char *who, int64_t first_row, int64_t nrows, const rtfe_csv_format_args *a, bool *uniform) {
   if (!a) return fail(-1, "%s: null argument", who);
   if (a->ntrks < 1 || a->ntrks > RTFE_MAXTRKS) return fail(-3, "%s: ntrks %d out of range", who, a->ntrks);
   if (a->perm) for (int k = 0; k < a->ntrks; ++k) if (a->perm[k] < 0 || a->perm[k] >= a->ntrks) return fail(-4, "%s: perm[%d] = %d out of range", who, k, a->perm[k]);
   if (first_row < 0 || nrows < 0 || first_row > INT64_MAX - nrows) return fail(-34, "%s: bad row range", who);
   const double bound = fabs((double)a->maxvolts) * 32768.0 / 32767.0 + (a->ntrks - 1) * fabs((double)a->stagger);
   if (!(bound < 1048576.0)) return fail(-46, "%s: maxvolts %g with stagger %g over %d tracks is outside the formatter's domain (below 2^20 volts)", who, (double)a->maxvolts, (double)a->stagger, a->ntrks);
   unsigned __int128 last = a->tstart_ns;
   if (nrows > 0) last += (unsigned __int128)(uint64_t)(first_row + nrows - 1) * a->tdelta_ns;
   if (nrows > 0 && last >= ((unsigned __int128)1 << 49)) return fail(-47, "%s: the window's last time is 2^49 ns or more", who);
   // a time prints three digits in front of its point while it ROUNDS below 1000 s: t + 5 < 10^12 ns
   *uniform = last + 5 < (unsigned __int128)1000000000000ull && bound < 99.0;
   return 0; }

extern "C" size_t rtfe_csv_format_max_bytes(int64_t nrows, int ntrks) { return nrows > 0 && ntrks > 0 ? (size_t)nrows * (size_t)co_max_line(ntrks) : 0; }
// (a workgroup formats at least (kCoLds - 16) / co_max_line(19) = 50 rows)
extern "C" size_t rtfe_csv_format_scratch_bytes(int64_t nrows) { return (size_t)((nrows > 0 ? nrows : 0) / co_lines_per_wg(co_max_line(RTFE_MAXTRKS)) + 1) * 8 + 16; }
extern "C" int rtfe_csv_format_path(int64_t first_row, int64_t nrows, const rtfe_csv_format_args *a) {
   bool uniform = false;
   const int rc = co_plan("rtfe_csv_format_path", first_row, nrows, a, &uniform);
   return rc ? rc : (uniform ? 1 : 0); }

extern "C" int rtfe_csv_format(const int16_t *d_rows, int64_t first_row, int64_t nrows, const rtfe_csv_format_args *a, void *d_text, size_t text_cap,
                               void *d_scratch, size_t scratch_bytes, rtfe_csv_text *d_out, void *stream) {
   if (!d_rows || !a || !d_text || !d_scratch || !d_out) return fail(-1, "rtfe_csv_format: null argument");
   bool uniform = false;
   const int rc = co_plan("rtfe_csv_format", first_row, nrows, a, &uniform);
   if (rc) return rc;
   if (((uintptr_t)d_text & 15) != 0) return fail(-31, "rtfe_csv_format: d_text must be 16-byte aligned");
   if (((uintptr_t)d_scratch & 7) != 0 || scratch_bytes < rtfe_csv_format_scratch_bytes(nrows)) return fail(-32, "rtfe_csv_format: scratch too small or misaligned");
   hipStream_t st = (hipStream_t)stream;
   CsvFormatArgs k;
   k.rows = d_rows; k.first_row = first_row; k.nrows = nrows;
   k.ntrks = a->ntrks; k.invert = a->invert != 0; k.maxvolts = a->maxvolts; k.stagger = a->stagger;
   k.tstart = a->tstart_ns; k.tdelta = a->tdelta_ns;
   k.perm_lo = k.perm_hi = 0;
   for (int c = 0; c < a->ntrks; ++c) {
      const unsigned long long col = (unsigned long long)(a->perm ? a->perm[c] : c);
      if (c < 12) k.perm_lo |= col << (5 * c); else k.perm_hi |= col << (5 * (c - 12)); }
   k.uniform_len = uniform ? (uint32_t)co_uniform_line(a->ntrks) : 0;
   k.lines = co_lines_per_wg(uniform ? co_uniform_line(a->ntrks) : co_max_line(a->ntrks));
   k.base = reinterpret_cast<const unsigned long long *>(d_scratch);
   k.text = reinterpret_cast<unsigned char *>(d_text); k.text_cap = text_cap;
   const int64_t nwg = (nrows + k.lines - 1) / k.lines;
   if (nwg > 0x7fffffffll) return fail(-34, "rtfe_csv_format: %lld rows are more than a launch takes", (long long)nrows);
   if (uniform) {
      hipLaunchKernelGGL(k_csvout_total, dim3(1), dim3(1), 0, st, d_out, (unsigned long long)nrows * k.uniform_len, (long long)nrows, nrows ? k.uniform_len : 0u, (unsigned long long)text_cap);
      if (nwg) hipLaunchKernelGGL(k_csvout_format<true>, dim3((unsigned)nwg), dim3(kCoWave), 0, st, k); }
   else {
      if (hipMemsetAsync(d_out, 0, sizeof(rtfe_csv_text), st) != hipSuccess) return fail(-30, "rtfe_csv_format: hipMemsetAsync failed");
      unsigned long long *sums = reinterpret_cast<unsigned long long *>(d_scratch);
      if (nwg) hipLaunchKernelGGL(k_csvout_len, dim3((unsigned)nwg), dim3(kCoWave), 0, st, k, sums, d_out);
      hipLaunchKernelGGL(k_csvout_scan, dim3(1), dim3(kCoScanThreads), 0, st, (uint32_t)nwg, sums, (long long)nrows, (unsigned long long)text_cap, d_out);
      if (nwg) hipLaunchKernelGGL(k_csvout_format<false>, dim3((unsigned)nwg), dim3(kCoWave), 0, st, k); }
   return launch_check("rtfe_csv_format"); }

// ---- a .tap image -> the interpreted text's body on the device (include/rt_frontend.h; kernels in rtfe_textfile.hip) ----
struct TxPlan {
   rt_text_options o;
   int doboth, narrow, lse, lines, maxline;
   uint16_t tail[kTxTail];
   unsigned long long max_stretches, max_lines, max_batches, max_bytes;
   size_t w_cnt, w_st, w_lines, w_base;      // the scratch's parts, in 8-byte words
};

// a line of n bytes behind its prefix (src/textfile.c:180-188, 260-275): the numbers with their -dataspace blanks, then - with a character type as well - the
// blanks that stand for the bytes the line lacks, two more without -dataspace, and a character a byte; '\n'
static int tx_tail(const rt_text_options &o, bool doboth, bool narrow, int n) {
   if (o.numtype == RT_NUM_NONE) return n + 1;
   const int alone = narrow ? 2 : 3;
   int len = o.numtype == RT_NUM_HEX ? 2 * n : o.numtype == RT_NUM_OCTAL ? alone * n : 6 * (n / 2) + (n & 1) * alone;
   if (o.dataspace > 0) {
      if (o.numtype != RT_NUM_OCTAL2) len += n / o.dataspace;
      else { for (int j = 2; j <= n; j += 2) len += j % o.dataspace == 0; if ((n & 1) && n % o.dataspace == 0) ++len; } }
   if (doboth) {
      const int missing = o.linesize - n;
      const int blanks = (o.dataspace ? missing / o.dataspace : 0) + missing * (o.numtype == RT_NUM_HEX || narrow ? 2 : 3);
      len += (blanks > 0 ? blanks : 0) + (o.dataspace == 0 ? 2 : 0) + n; }
   return len + 1; }

static int tx_plan(const char *who, const rtfe_text_item *items, int64_t nitems, uint64_t image_bytes, uint64_t nlinefeeds, const rtfe_text_options *in, TxPlan *p) {
   if (!in || (!items && nitems > 0)) return fail(-1, "%s: null argument", who);
   if (nitems < 0 || nitems > 0x7fffffffll) return fail(-34, "%s: %lld items are more than a launch takes", who, (long long)nitems);
   const rt_text_options raw = { in->numtype, in->chartype, in->linesize, in->dataspace, in->linefeed, in->ntrks };
   const int bad = rt_text_resolve(&raw, &p->o);
   if (bad) return fail(-50, "%s: text option %d (1 number type, 2 character type, 3 linesize, 4 dataspace) is out of range", who, bad);
   if (in->verbose) return fail(-51, "%s: the verbose layout's block lines are the host's strings: the decode path writes its text on the host", who);
   if (p->o.numtype == RT_NUM_NONE && p->o.chartype == RT_CHAR_NONE)
      return fail(-52, "%s: without a number or a character type the text is a list of block sizes, which is sequential: the host writes it", who);
   p->doboth = p->o.numtype != RT_NUM_NONE && p->o.chartype != RT_CHAR_NONE;
   p->narrow = p->o.ntrks <= 7;
   p->lse = p->o.numtype == RT_NUM_OCTAL2 ? (p->o.linesize + 1) & ~1 : p->o.linesize;
   int tailmax = 0;
   for (int n = 0; n < kTxTail; ++n) {
      const int t = n <= p->lse ? tx_tail(p->o, p->doboth, p->narrow, n) : 0;
      p->tail[n] = (uint16_t)t;
      const int wide = !p->narrow ? 0 : p->o.numtype == RT_NUM_OCTAL ? n : p->o.numtype == RT_NUM_OCTAL2 ? (n & 1) : 0;
      if (t + wide > tailmax) tailmax = t + wide; }
   p->maxline = 9 + tailmax;
   if (p->maxline < 40) p->maxline = 40;                                       // (a message line)
   p->lines = (kTxLds - 16) / p->maxline < kTxWave ? (kTxLds - 16) / p->maxline : kTxWave;
   unsigned long long lines = 0, bytes = 0;
   const unsigned long long full = 7ull + p->tail[p->lse];
   for (int64_t i = 0; i < nitems; ++i) {
      const rtfe_text_item &it = items[i];
      if (it.kind == RT_TAP_MARK) { ++lines; bytes += strlen(RT_TAP_MARK_TEXT); continue; }
      if (it.kind == RT_TAP_MESSAGE) {
         if (it.flag > 1) return fail(-53, "%s: item %lld: no message %d", who, (long long)i, (int)it.flag);
         ++lines; bytes += strlen(rt_tap_messages[it.flag]); continue; }
      if (it.kind != RT_TAP_RECORD) return fail(-53, "%s: item %lld is of kind %d", who, (long long)i, (int)it.kind);
      if (it.length < 1 || it.length >= RT_TEXT_MAXBLOCK) return fail(-54, "%s: item %lld: a record of %u bytes", who, (long long)i, it.length);
      if (it.offset > image_bytes || image_bytes - it.offset < it.length) return fail(-55, "%s: item %lld lies outside the image", who, (long long)i);
      const unsigned long long nl = (it.length + (unsigned)p->lse - 1) / (unsigned)p->lse, last = it.length - (nl - 1) * (unsigned)p->lse;
      lines += nl;
      bytes += (it.length < 10000u ? 7 : it.length < 100000u ? 8 : 9) + (nl - 1) * full + p->tail[last];
      if (p->narrow && p->o.numtype == RT_NUM_OCTAL) bytes += it.length; else if (p->narrow && p->o.numtype == RT_NUM_OCTAL2) bytes += 1; }
   const unsigned long long extra = p->o.linefeed ? nlinefeeds + (unsigned long long)nitems : 0;      // a linefeed adds a stretch, a stretch at most a line
   p->max_stretches = (unsigned long long)nitems + extra;
   p->max_lines = lines + extra;
   p->max_batches = (p->max_lines + (unsigned)p->lines - 1) / (unsigned)p->lines;
   p->max_bytes = bytes + extra * (unsigned long long)p->maxline;
   p->w_cnt = p->o.linefeed ? (size_t)nitems + 1 : 0;
   p->w_st = p->o.linefeed ? (size_t)p->max_stretches : 0;
   p->w_lines = (size_t)p->max_stretches + 1;
   p->w_base = (size_t)p->max_batches + 1;
   return 0; }

extern "C" size_t rtfe_text_format_max_bytes(const rtfe_text_item *items, int64_t nitems, uint64_t nlinefeeds, const rtfe_text_options *o) {
   TxPlan p;
   return tx_plan("rtfe_text_format_max_bytes", items, nitems, UINT64_MAX, nlinefeeds, o, &p) ? 0 : (size_t)p.max_bytes; }
extern "C" size_t rtfe_text_format_scratch_bytes(const rtfe_text_item *items, int64_t nitems, uint64_t nlinefeeds, const rtfe_text_options *o) {
   TxPlan p;
   return tx_plan("rtfe_text_format_scratch_bytes", items, nitems, UINT64_MAX, nlinefeeds, o, &p) ? 0 : (p.w_cnt + p.w_st + p.w_lines + p.w_base) * 8 + 16; }

extern "C" int rtfe_text_format(const void *d_image, uint64_t image_bytes, const rtfe_text_item *items, const rtfe_text_item *d_items, int64_t nitems, uint64_t nlinefeeds,
                                const rtfe_text_options *o, void *d_text, size_t text_cap, void *d_scratch, size_t scratch_bytes, rtfe_text_out *d_out, void *stream) {
   static_assert(sizeof(rtfe_text_item) == sizeof(rt_tap_item) && sizeof(rtfe_text_item) == 16, "one item layout");
   if (!d_image || !d_items || !d_text || !d_scratch || !d_out) return fail(-1, "rtfe_text_format: null argument");
   TxPlan p;
   const int rc = tx_plan("rtfe_text_format", items, nitems, image_bytes, nlinefeeds, o, &p);
   if (rc) return rc;
   if (((uintptr_t)d_text & 15) != 0) return fail(-31, "rtfe_text_format: d_text must be 16-byte aligned");
   if (((uintptr_t)d_scratch & 7) != 0 || scratch_bytes < (p.w_cnt + p.w_st + p.w_lines + p.w_base) * 8 + 16) return fail(-32, "rtfe_text_format: scratch too small or misaligned");
   hipStream_t st = (hipStream_t)stream;
   TxArgs k;
   k.image = reinterpret_cast<const unsigned char *>(d_image); k.items = d_items; k.nitems = nitems;
   k.numtype = p.o.numtype; k.doboth = p.doboth; k.linesize = p.o.linesize; k.lse = p.lse; k.dataspace = p.o.dataspace; k.linefeed = p.o.linefeed; k.narrow = p.narrow;
   k.lines = p.lines; k.max_stretches = p.max_stretches; k.max_batches = p.max_batches;
   k.cnt = reinterpret_cast<unsigned long long *>(d_scratch); k.st = k.cnt + p.w_cnt; k.lines_v = k.st + p.w_st; k.base = k.lines_v + p.w_lines;
   k.out_bytes = reinterpret_cast<unsigned long long *>(&d_out->bytes); k.out_lines = reinterpret_cast<unsigned long long *>(&d_out->lines);
   k.out_stretches = reinterpret_cast<unsigned long long *>(&d_out->stretches); k.out_flags = &d_out->flags;
   k.text = reinterpret_cast<unsigned char *>(d_text); k.text_cap = text_cap;
   memcpy(k.tail, p.tail, sizeof k.tail);
   rt_text_char_table(p.o.chartype, k.table);
   if (hipMemsetAsync(d_out, 0, sizeof(rtfe_text_out), st) != hipSuccess) return fail(-30, "rtfe_text_format: hipMemsetAsync failed");
   if (nitems == 0) return launch_check("rtfe_text_format");
   if (p.o.linefeed) {
      hipLaunchKernelGGL(k_tx_stretch<false>, dim3((unsigned)nitems), dim3(kTxWave), 0, st, k);
      hipLaunchKernelGGL(k_tx_scan, dim3(1), dim3(kTxScanThreads), 0, st, k.cnt, (unsigned long long)nitems, (const unsigned long long *)nullptr, 1ull, (unsigned long long)nitems,
                         k.out_stretches, p.max_stretches, k.out_flags, (uint32_t)RTFE_TEXT_SCRATCH_FULL);
      hipLaunchKernelGGL(k_tx_stretch<true>, dim3((unsigned)nitems), dim3(kTxWave), 0, st, k); }
   hipLaunchKernelGGL(k_tx_measure, dim3((unsigned)((p.max_stretches + 255) / 256)), dim3(256), 0, st, k);
   hipLaunchKernelGGL(k_tx_scan, dim3(1), dim3(kTxScanThreads), 0, st, k.lines_v, (unsigned long long)nitems, p.o.linefeed ? (const unsigned long long *)k.out_stretches : nullptr, 1ull,
                      p.max_stretches, k.out_lines, ~0ull, (uint32_t *)nullptr, 0u);
   const unsigned grid = (unsigned)(p.max_batches < (unsigned long long)kTxMaxGrid ? p.max_batches : (unsigned long long)kTxMaxGrid);
   hipLaunchKernelGGL(k_tx_len, dim3(grid), dim3(kTxWave), 0, st, k);
   hipLaunchKernelGGL(k_tx_scan, dim3(1), dim3(kTxScanThreads), 0, st, k.base, 0ull, (const unsigned long long *)k.out_lines, (unsigned long long)p.lines, p.max_batches,
                      k.out_bytes, (unsigned long long)text_cap, k.out_flags, (uint32_t)RTFE_TEXT_FULL);
   hipLaunchKernelGGL(k_tx_format, dim3(grid), dim3(kTxWave), 0, st, k);
   return launch_check("rtfe_text_format"); }

// ---- a slot stream and a block table -> the tape's rows on the device (include/rt_frontend.h; the kernel is rtfe_tapewrite.hip) ----
extern "C" int64_t rtfe_tape_render_span_rows(int ntrks) { return ntrks >= 1 && ntrks <= RTFE_MAXTRKS ? kTwSpanRows : 0; }

extern "C" int rtfe_tape_render(const rtfe_tape_slot *d_slots, int64_t nslots, const rtfe_tape_block *blocks, const rtfe_tape_block *d_blocks, int64_t nblocks,
                                const rtfe_tape_params *p, int64_t first_row, int64_t nrows, int16_t *d_rows, void *stream) {
   if (!p || !d_rows) return fail(-1, "rtfe_tape_render: null argument");
   if (nslots < 0 || nblocks < 0 || first_row < 0 || nrows < 0 || first_row > INT64_MAX - nrows) return fail(-34, "rtfe_tape_render: a negative count or row (nslots %lld, nblocks %lld, first_row %lld, nrows %lld)", (long long)nslots, (long long)nblocks, (long long)first_row, (long long)nrows);
   if ((nslots > 0 && !d_slots) || (nblocks > 0 && (!blocks || !d_blocks))) return fail(-1, "rtfe_tape_render: null argument");
   if (p->ntrks < 1 || p->ntrks > RTFE_MAXTRKS) return fail(-3, "rtfe_tape_render: ntrks %d out of range", p->ntrks);
   if (((uintptr_t)d_rows & 15) != 0) return fail(-31, "rtfe_tape_render: d_rows must be 16-byte aligned");
   if (!(p->spb > 0 && std::isfinite(p->spb)) || !(p->w > 0 && std::isfinite(p->w)) || !std::isfinite(p->edge) || !(p->maxvolts > 0 && std::isfinite(p->maxvolts)) ||
       !(p->noise_mv >= 0 && std::isfinite(p->noise_mv)) || !(p->jitter >= 0 && std::isfinite(p->jitter)) || p->pitch_shift < 0 || p->pitch_shift > 1)
      return fail(-62, "rtfe_tape_render: spb %g, w %g, edge %g, maxvolts %g, noise %g mV, jitter %g, pitch shift %d: not a tape", p->spb, p->w, p->edge, p->maxvolts, p->noise_mv, p->jitter, p->pitch_shift);
   double skew = 0;
   for (int t = 0; t < p->ntrks; ++t) {
      if (!std::isfinite(p->amp[t]) || !std::isfinite(p->skew[t])) return fail(-62, "rtfe_tape_render: track %d: amplitude %g, skew %g", t, p->amp[t], p->skew[t]);
      if (fabs(p->skew[t]) > skew) skew = fabs(p->skew[t]); }
   if (p->K < 0 || p->K > RTFE_TAPE_MAX_REACH) return fail(-60, "rtfe_tape_render: a reach of %d rows (0 .. %d)", p->K, RTFE_TAPE_MAX_REACH);
   TapeArgs k;
   const double astray = ceil((skew + RT_TW_GMAX * p->jitter) * p->spb);                 // rows a transition can lie from its slot's nominal place
   k.slots_per_row = 1.0 / (p->spb * (p->pitch_shift ? 0.5 : 1.0));
   const double need = (kTwSpanRows + 2.0 * (p->K + 2.0 + astray)) * k.slots_per_row + 7.0;
   if (!(need <= kTwSlotCap)) return fail(-60, "rtfe_tape_render: %.3f rows a slot with a reach of %d rows and %.0f of skew and jitter: a span needs %.0f slots, the kernel stages %d", 1.0 / k.slots_per_row, p->K, astray, need, kTwSlotCap);
   int64_t row = 0;
   for (int64_t b = 0; b < nblocks; ++b) {
      const rtfe_tape_block &B = blocks[b];
      if (B.first_row < row || B.rows < 1 || B.rows > INT64_MAX - B.first_row || B.first_slot < 0 || B.nslots < 0 || B.nslots > 0x7fffffffll || B.first_slot > nslots || B.nslots > nslots - B.first_slot)
         return fail(-61, "rtfe_tape_render: block %lld of the table (rows %lld + %lld, slots %lld + %lld of %lld) is out of order or out of range", (long long)b, (long long)B.first_row, (long long)B.rows, (long long)B.first_slot, (long long)B.nslots, (long long)nslots);
      row = B.first_row + B.rows; }
   if (nrows == 0) return 0;
   k.span0 = first_row / kTwSpanRows;
   const int64_t nwg = (first_row + nrows - 1) / kTwSpanRows - k.span0 + 1;
   if (nwg > 0x7fffffffll) return fail(-34, "rtfe_tape_render: %lld rows are more than a launch takes", (long long)nrows);
   k.slots = d_slots; k.blocks = d_blocks; k.nblocks = nblocks; k.first_row = first_row; k.nrows = nrows; k.rows = d_rows;
   k.reach = (long long)(p->K + 2 + astray);
   k.lead_rows = (RT_TW_LEAD + 0.5) * p->spb;
   k.p = *p;
   hipLaunchKernelGGL(k_tape_render, dim3((unsigned)nwg), dim3(kTwThreads), 0, (hipStream_t)stream, k);
   return launch_check("rtfe_tape_render"); }
