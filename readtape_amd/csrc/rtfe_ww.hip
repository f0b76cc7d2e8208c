// rtfe_ww.hip — k_ww: the peak detector for Whirlwind tapes, with detector state that is handed in and out; k_ww_det (below): the same for the
// reference's other three detectors (-zeros, -differentiate -zeros, -differentiate).
//
// Whirlwind blocks can be one bit apart, so the reference never restarts its detector between them (src/readtape.c:1674,
// src/decode_ww.c:31-49): the peak window's ring, its extremes, the blind countdown and the AGC state all carry over.  What a
// new block attempt does do is zero t_lastpeak, and process_sample (src/decoder.c:855-861) then RE-SEEDS each track - one track
// per sample, in track order, the later tracks sitting out until their turn - by overwriting ring slot 0 with the current sample
// and setting the window's extremes to it, while the ring's indices and its other slots keep what they held.  From then on the
// window is not the last W samples any more, and WHERE an attempt starts is the host decoder's decision (its clock average
// decides when the clock has stopped).  So this kernel is the literal detector - ring, stale extremes and all - run by one lane
// per track over the rows it is given, from a state blob the host hands in, to a state blob it hands back:
//      rtfe_ww_scan(first_row, nrows, seed_row0, state_in) -> events of [first_row, first_row + nrows), state after the last row.
// The host replay asks for rows in chunks, and - when its decoder ends a block at row r - for the state after r (a second, shorter
// scan of the same chunk), which is where the next attempt starts.  The tapes are short (100 BPI) and there is one chain per tape:
// this path is exact, not fast.  Included behind rtfe_kernels.hip (volt, refine_code, agc_after_peak, update_thresholds).

namespace rtfe {

constexpr int kWwRing = 64;           // >= RT_PKWW_MAX_WIDTH (50)

__global__ void __launch_bounds__(64) k_ww(const DevCfg *__restrict__ cfgp, const int16_t *__restrict__ rows, long long nrows_total, long long row_base,
                                          long long first_row, long long nscan, long long seed_row0,
                                          const rtfe_ww_track *__restrict__ state_in, rtfe_ww_track *__restrict__ state_out,
                                          uint32_t *__restrict__ counts, rtfe_event *__restrict__ events, long long cap, unsigned int *__restrict__ flags_out) {
   __shared__ short s_ring[RTFE_MAXTRKS][kWwRing];
   __shared__ float s_heights[RTFE_MAXTRKS][10];
   const DevCfg &cfg = *cfgp;
   const int t = threadIdx.x;
   if (t >= cfg.ntrks) return;
   const DevParm &P = cfg.parm[0];
   const int W = P.W;
   const float mv = cfg.maxvolts;
   const int col = cfg.trk_to_head[t];
   const int sgn = cfg.invert ? -1 : 1;
   rtfe_ww_track S = state_in[t];
   short *ring = s_ring[t];
   for (int i = 0; i < kWwRing; ++i) ring[i] = S.ring[i];
   // -invert: v = -x reaches +32768 (the reference negates the voltage, src/readtape.c:1421) and never -32768, so the ring's 16 bits - in LDS
   // and in the state blob - hold that one value as -32768 and every read turns it back (zc_code)
   const int rail = zc_rail(&cfg);
   auto rd = [&](int i) -> int { return zc_code(ring[i], rail); };
   float *heights = s_heights[t];
   for (int i = 0; i < 10; ++i) heights[i] = S.heights[i];
   Walker w = {};
   w.agc_gain = S.agc_gain; w.v_avg_height = S.v_avg_height; w.v_lasttop = S.v_lasttop; w.v_lastbot = S.v_lastbot;
   w.v_top = S.v_top; w.v_bot = S.v_bot; w.peakcount = S.peakcount; w.heightndx = S.heightndx;
   int left = S.left, right = S.right, maxv = S.maxv, minv = S.minv, countdown = S.countdown;
   const int delay = S.delay < 0 ? 0 : (S.delay > 50 ? 50 : S.delay);      // (MAXSKEWSAMP)
   unsigned int nev = 0, fl = 0;
   rtfe_event *out = events + (size_t)t * cap;
   const long long end = first_row + nscan < nrows_total ? first_row + nscan : nrows_total;
   for (long long n = first_row; n < end && !(fl & (RTFE_F_DETECTOR_FATAL | RTFE_F_AGC_FATAL)); ++n) {
      if (n < seed_row0 + t) continue;                               // the tracks in front of this one are being re-seeded: it sits the row out
      const long long src = (row_base + n < delay || n < delay) ? n : n - delay;    // the deskew FIFO runs from the tape's first row: undelayed until it has filled (src/decoder.c:820-830)
      const int v = sgn * (int)rows[src * cfg.ntrks + col];
      if (n == seed_row0 + t) {                                      // src/decoder.c:855-861: slot 0, both extremes; indices and the other slots stay
         ring[0] = (short)v; maxv = minv = v;
         continue; }
      // ---- lookfor_peak, src/decoder.c:751-810 ----
      int old_left = 0;
      if (++right >= W) right = 0;
      if (right == left) { old_left = rd(left); if (++left >= W) left = 0; }
      ring[right] = (short)v;
      if (v > maxv) maxv = v;
      if (old_left == maxv || old_left == minv) {                    // (the reference compares floats: 0.0f == volt(0), and == on volts is == on codes)
         int mx = -0x7fffffff, mn = 0x7fffffff;
         for (int ndx = left;;) {
            const int u = rd(ndx);
            mx = max(mx, u); mn = min(mn, u);
            if (ndx == right) break;
            if (++ndx >= W) ndx = 0; }
         maxv = mx; minv = mn; }
      if (countdown) { --countdown; continue; }
      if (!(w.agc_gain > 0)) {                                       // src/decoder.c:782: fatal in the reference; the marker tells the replay where
         fl |= RTFE_F_AGC_FATAL;
         if (nev < cap) { rtfe_event e = {}; e.sample = (uint32_t)(n - first_row); e.trk = (uint8_t)t; e.flags = RTFE_EV_FATAL; out[nev] = e; }
         ++nev;
         break; }
      const float rise = P.rise * (w.v_avg_height / 4.0f) / w.agc_gain;
      const float reqmin = P.min_peak * (w.v_avg_height / 4.0f) / w.agc_gain;
      const float vl = volt(rd(left), mv), vr = volt(rd(right), mv);
      const float vmax = volt(maxv, mv), vmin = volt(minv, mv);
      const bool top = vmax > vl + rise && vmax > vr + rise && (reqmin == 0 || vmax > reqmin);
      const bool bot = !top && vmin < vl - rise && vmin < vr - rise && (reqmin == 0 || vmin < -reqmin);
      if (!top && !bot) continue;
      // ---- refine_peak, src/decoder.c:700-749: the first window element equal to the extreme, its neighbours ----
      const int val = top ? maxv : minv;
      int ld = 1, ndx = left, prev = -1;
      bool found = false;
      for (;;) {
         if (rd(ndx) == val) { found = true; break; }
         if (ndx == right) break;
         prev = ndx;
         ++ld;
         if (++ndx >= W) ndx = 0; }
      if (!found || prev < 0 || !(ld < W)) { fl |= RTFE_F_DETECTOR_FATAL; break; }         // src/decoder.c:709-710, 748
      int nxt = ndx + 1; if (nxt >= W) nxt = 0;
      const int adjcode = refine_code(&cfg, val, rd(prev), rd(nxt), w.agc_gain, top);
      if (nev < cap) {
         rtfe_event e;
         e.sample = (uint32_t)(n - first_row);
         const float vp = volt(val, mv);
         e.v_peak = (cfg.invert && vp == 0.0f) ? -0.0f : vp;
         e.agc_gain = w.agc_gain;
         e.trk = (uint8_t)t;
         e.flags = (uint8_t)((top ? 0 : 1) | (adjcode << 1));
         e.left_distance = (uint8_t)ld;
         e.parmset = 0;
         out[nev] = e; }
      else fl |= RTFE_F_EVENT_OVERFLOW;
      ++nev;
      if (top) w.v_top = volt(val, mv); else w.v_bot = volt(val, mv);
      agc_after_peak(w, &cfg, P, heights, top, 0.0);                 // Whirlwind: every pulse edge adjusts the gain (src/decode_ww.c:175,194)
      countdown = ld; }                                              // src/decoder.c:741
   // ---- the state after the last row ----
   for (int i = 0; i < kWwRing; ++i) S.ring[i] = ring[i];
   for (int i = 0; i < 10; ++i) S.heights[i] = heights[i];
   S.left = left; S.right = right; S.maxv = maxv; S.minv = minv; S.countdown = countdown;
   S.agc_gain = w.agc_gain; S.v_avg_height = w.v_avg_height; S.v_lasttop = w.v_lasttop; S.v_lastbot = w.v_lastbot;
   S.v_top = w.v_top; S.v_bot = w.v_bot; S.peakcount = w.peakcount; S.heightndx = w.heightndx;
   state_out[t] = S;
   counts[t] = nev < cap ? nev : (unsigned int)cap;
   if (fl) atomicOr(flags_out, fl); }

// ---- k_ww_det: Whirlwind with -zeros and / or -differentiate (include/rt_frontend.h: rtfe_ww_detector_scan) ----
// The same contract as k_ww - rows [first_row, first_row + nscan), state blob in, state blob out, one lane per track, the tracks of an attempt
// re-seeded one per row from seed_row0 - for the reference's other three detectors.  On its seed row and in front of it a track runs NO detector
// (the `break` of src/decoder.c:861: the zero detectors' v_prev and extremes are not touched there), but differentiate() has run on those rows
// (src/readtape.c:1422): what a row is differentiated against is the row in front of it in the file, whatever the detector did with it - except
// row 0 of the tape, which meets v_raw_row0 (0; after the -deskew rewind the last row the pre-pass read).  differentiate() runs in front of the
// deskew delay line (src/decoder.c:820-830), so the detector at row n sees the differentiated sample of row n - delay.
// Rows the detectors remember are absolute rows of the tape (row_base + n).

// differentiate() for one sample, the float operations of walk_diffzeros / differentiate_tile (src/readtape.c:1383-1388)
__device__ __forceinline__ float ww_diff(int raw, int prev, float mv, int spb) {
   float delta = volt(raw, mv) - volt(prev, mv);
   if (delta < 0.05f && delta > -0.05f) delta = 0;
   return delta * 0.4f * spb; }

__device__ __forceinline__ void ww_put(rtfe_ww_event *out, unsigned int nev, long long cap, unsigned int &fl, long long n_rel, int t, float v_peak, float gain,
                                       int flags, int ld, float v_other, unsigned int has_zero, long long back_first, long long back_last) {
   if ((long long)nev >= cap) { fl |= RTFE_F_EVENT_OVERFLOW; return; }
   rtfe_ww_event e;
   e.ev.sample = (uint32_t)n_rel; e.ev.v_peak = v_peak; e.ev.agc_gain = gain; e.ev.trk = (uint8_t)t; e.ev.flags = (uint8_t)flags;
   e.ev.left_distance = (uint8_t)ld; e.ev.parmset = 0;
   e.v_other = v_other; e.has_zero = has_zero; e.back_first = back_first; e.back_last = back_last;
   out[nev] = e; }

__global__ void __launch_bounds__(64) k_ww_det(const DevCfg *__restrict__ cfgp, const int16_t *__restrict__ rows, long long nrows_total, long long row_base,
                                              long long first_row, long long nscan, long long seed_row0, int kind,
                                              const rtfe_ww_dtrack *__restrict__ state_in, rtfe_ww_dtrack *__restrict__ state_out,
                                              uint32_t *__restrict__ counts, rtfe_ww_event *__restrict__ events, long long cap, unsigned int *__restrict__ flags_out) {
   __shared__ float s_ring[RTFE_MAXTRKS][kWwRing];
   __shared__ float s_heights[RTFE_MAXTRKS][10];
   const DevCfg &cfg = *cfgp;
   const int t = threadIdx.x;
   if (t >= cfg.ntrks) return;
   const DevParm &P = cfg.parm[0];
   const int W = P.W;
   const float mv = cfg.maxvolts;
   const int col = cfg.trk_to_head[t], ntrks = cfg.ntrks;
   const int sgn = cfg.invert ? -1 : 1;
   const int spb = cfg.samples_per_bit;
   rtfe_ww_dtrack S = state_in[t];
   if (S.kind != kind) {                                             // a blob of another detector: nothing is scanned, the state goes back as it came
      state_out[t] = S; counts[t] = 0;
      atomicOr(flags_out, (unsigned int)RTFE_F_STATE_KIND);
      return; }
   const int delay = S.delay < 0 ? 0 : (S.delay > 50 ? 50 : S.delay);      // (MAXSKEWSAMP)
   unsigned int nev = 0, fl = 0;
   rtfe_ww_event *out = events + (size_t)t * cap;
   const long long end = first_row + nscan < nrows_total ? first_row + nscan : nrows_total;
   const long long seed = seed_row0 + t;
   // the sample the detector sees at row n, as a code (undifferentiated) / its row (differentiated): the deskew FIFO runs from the tape's first row
   auto src_of = [&](long long n) { return (row_base + n < delay || n < delay) ? n : n - delay; };
   auto code_at = [&](long long r) { return sgn * (int)rows[r * ntrks + col]; };
   auto diff_at = [&](long long r) { return ww_diff(code_at(r), (row_base + r == 0 || r == 0) ? S.v_raw_row0 : code_at(r - 1), mv, spb); };

   if (kind == RTFE_WW_ZEROS) {                                      // ---- lookfor_zerocrossing, src/decoder.c:617-649 (zc_row) ----
      ZcState z; z.prev = S.z_prev; z.top = S.z_top; z.bot = S.z_bot; z.up = S.up_pending != 0; z.dn = S.dn_pending != 0; z.ttop = S.row_top; z.tbot = S.row_bot;
      const int Pk = cfg.zc_peak_i;
      for (long long n = first_row; n < end; ++n) {
         if (n <= seed) continue;
         const int v = code_at(src_of(n));
         bool up = false; long long cross = 0;
         if (zc_row(z, v, row_base + n, Pk, up, cross)) {
            ww_put(out, nev, cap, fl, n - first_row, t, volt(v, mv), 1.0f, up ? 0 : 1, 0, 0.0f, 0, row_base + n - cross, 0);
            ++nev; } }
      S.z_prev = z.prev; S.z_top = z.top; S.z_bot = z.bot; S.up_pending = z.up; S.dn_pending = z.dn; S.row_top = z.ttop; S.row_bot = z.tbot; }

   else if (kind == RTFE_WW_DIFFZEROS) {                             // ---- lookfor_differentiated_zerocrossing, src/decoder.c:654-683 (the body of walk_diffzeros) ----
      float ztop = S.zf_top, zbot = S.zf_bot;
      bool upp = S.up_pending != 0, dnp = S.dn_pending != 0, have = S.have_zero != 0;
      long long fz = S.row_firstzero, lz = S.row_lastzero;
      for (long long n = first_row; n < end; ++n) {
         if (n <= seed) continue;
         const float v = diff_at(src_of(n));
         const long long a = row_base + n;
         if (v > 0) {
            if (ztop < v) ztop = v;
            if (upp) {
               ww_put(out, nev, cap, fl, n - first_row, t, ztop, 1.0f, 0, 0, zbot, have ? 1u : 0u, have ? a - fz : 0, have ? a - lz : 0);
               ++nev;
               upp = false; have = false; }
            if (v > 0.2f) { dnp = true; have = false; zbot = 0; } }
         else if (v < 0) {
            if (zbot > v) zbot = v;
            if (dnp) {
               ww_put(out, nev, cap, fl, n - first_row, t, zbot, 1.0f, 1, 0, ztop, have ? 1u : 0u, have ? a - fz : 0, have ? a - lz : 0);
               ++nev;
               dnp = false; have = false; }
            if (v < -0.2f) { upp = true; have = false; ztop = 0; } }
         else { lz = a; if (!have) { fz = a; have = true; } } }
      S.zf_top = ztop; S.zf_bot = zbot; S.up_pending = upp; S.dn_pending = dnp; S.have_zero = have; S.row_firstzero = fz; S.row_lastzero = lz; }

   else {                                                            // ---- RTFE_WW_DIFFPEAKS: lookfor_peak / refine_peak on the differentiated signal (k_ww, on floats) ----
      float *ring = s_ring[t];
      for (int i = 0; i < kWwRing; ++i) ring[i] = S.ring[i];
      float *heights = s_heights[t];
      for (int i = 0; i < 10; ++i) heights[i] = S.heights[i];
      Walker w = {};
      w.agc_gain = S.agc_gain; w.v_avg_height = S.v_avg_height; w.v_lasttop = S.v_lasttop; w.v_lastbot = S.v_lastbot;
      w.v_top = S.v_top; w.v_bot = S.v_bot; w.peakcount = S.peakcount; w.heightndx = S.heightndx;
      int left = S.left, right = S.right, countdown = S.countdown;
      float maxv = S.maxv, minv = S.minv;
      for (long long n = first_row; n < end && !(fl & (RTFE_F_DETECTOR_FATAL | RTFE_F_AGC_FATAL)); ++n) {
         if (n < seed) continue;
         const float v = diff_at(src_of(n));
         if (n == seed) {                                            // src/decoder.c:855-861: slot 0, both extremes; indices and the other slots stay
            ring[0] = v; maxv = minv = v;
            continue; }
         float old_left = 0;
         if (++right >= W) right = 0;
         if (right == left) { old_left = ring[left]; if (++left >= W) left = 0; }
         ring[right] = v;
         if (v > maxv) maxv = v;
         if (old_left == maxv || old_left == minv) {
            float mx = -100, mn = 100;
            for (int ndx = left;;) {
               const float u = ring[ndx];
               mx = mx > u ? mx : u; mn = mn < u ? mn : u;
               if (ndx == right) break;
               if (++ndx >= W) ndx = 0; }
            maxv = mx; minv = mn; }
         if (countdown) { --countdown; continue; }
         if (!(w.agc_gain > 0)) {                                    // src/decoder.c:782: fatal in the reference; the marker tells the replay where
            fl |= RTFE_F_AGC_FATAL;
            ww_put(out, nev, cap, fl, n - first_row, t, 0.0f, 0.0f, RTFE_EV_FATAL, 0, 0.0f, 0, 0, 0);
            ++nev;
            break; }
         const float rise = P.rise * (w.v_avg_height / 4.0f) / w.agc_gain;
         const float reqmin = P.min_peak * (w.v_avg_height / 4.0f) / w.agc_gain;
         const float vl = ring[left], vr = ring[right];
         const bool top = maxv > vl + rise && maxv > vr + rise && (reqmin == 0 || maxv > reqmin);
         const bool bot = !top && minv < vl - rise && minv < vr - rise && (reqmin == 0 || minv < -reqmin);
         if (!top && !bot) continue;
         // ---- refine_peak, src/decoder.c:700-749 (the float comparisons of walk_diffpeak) ----
         const float val = top ? maxv : minv;
         int ld = 1, ndx = left, prev = -1;
         bool found = false;
         for (;;) {
            if (ring[ndx] == val) { found = true; break; }
            if (ndx == right) break;
            prev = ndx;
            ++ld;
            if (++ndx >= W) ndx = 0; }
         if (!found || prev < 0 || !(ld < W)) { fl |= RTFE_F_DETECTOR_FATAL; break; }         // src/decoder.c:709-710, 748
         int nxt = ndx + 1; if (nxt >= W) nxt = 0;
         const float vp = ring[prev], vn = ring[nxt];
         int adjcode = 0;
         if (top) {
            const float lim = val - 0.005f / w.agc_gain;
            if (vp > lim && vn < lim) adjcode = 1; else if (vn > lim && vp < lim) adjcode = 2; }
         else {
            const float lim = val + 0.005f / w.agc_gain;
            if (vp < lim && vn > lim) adjcode = 1; else if (vn < lim && vp > lim) adjcode = 2; }
         ww_put(out, nev, cap, fl, n - first_row, t, val, w.agc_gain, (top ? 0 : 1) | (adjcode << 1), ld, 0.0f, 0, 0, 0);
         ++nev;
         if (top) w.v_top = val; else w.v_bot = val;
         agc_after_peak(w, &cfg, P, heights, top, 0.0);
         countdown = ld; }
      for (int i = 0; i < kWwRing; ++i) S.ring[i] = ring[i];
      for (int i = 0; i < 10; ++i) S.heights[i] = heights[i];
      S.left = left; S.right = right; S.maxv = maxv; S.minv = minv; S.countdown = countdown;
      S.agc_gain = w.agc_gain; S.v_avg_height = w.v_avg_height; S.v_lasttop = w.v_lasttop; S.v_lastbot = w.v_lastbot;
      S.v_top = w.v_top; S.v_bot = w.v_bot; S.peakcount = w.peakcount; S.heightndx = w.heightndx; }

   if (end > first_row) S.v_last_raw = code_at(end - 1);             // differentiate() has read every row, detector or not (src/readtape.c:1387)
   state_out[t] = S;
   counts[t] = (long long)nev < cap ? nev : (unsigned int)cap;
   if (fl) atomicOr(flags_out, fl); }

}  // namespace rtfe
