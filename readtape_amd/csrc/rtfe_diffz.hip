// rtfe_diffz.hip — k_diffz: the -zeros -differentiate front end (lookfor_differentiated_zerocrossing, src/decoder.c:654-683, on
// differentiate()'s output, src/readtape.c:1383-1388) as a kernel of its own.
//
// Once differentiated, the detector is a transducer on three states - no crossing pending, one upward, one downward - with no AGC,
// no window and no feedback.  What a row does depends on the class of its differentiated sample v alone:
//   v >  0.2     every state goes to "downward pending"; an event if upward was pending
//   0 < v <= 0.2 "upward pending" goes to "none" with an event; the other two stay
//   v == 0       identity (the row is noted as the first / last exact zero since the last arming row or event)
//   v <  0       the mirror images.
// The two flags of the reference are never both set behind a row (a positive row clears "up", a negative one "down", and only those
// set the other), v_top is 0 while "up" is pending (zeroed when armed, and any positive sample fires), so an event's v_peak is the
// confirming sample itself, and t_firstzero is reset at every arming row and every event: d1 / d2 count the zeros since then.
// A stretch of rows is therefore a map on the three entry states.  Its first row with |v| > 0.2 MERGES them: behind it nothing
// depends on the entry state.  In front of it a pending crossing can only be confirmed (once, by the first sample of its sign, the
// merging row included) - so one walk from "none" that notes "a positive / negative sample up to the merging row" is the whole map:
//   events(entry) = events(none) + (entry == up && seen_pos) + (entry == dn && seen_neg)
//   exit(entry)   = merged ? exit(none) : (confirmed ? none : entry)
//   zeros carried = merged ? those of the walk : (still pending ? entry's first zero, else the stretch's; the stretch's last zero, else entry's)
// and these maps compose associatively, exactly, for every input: no warm-up rows, no join check, no repair.
//
// A burst is one workgroup's (persistent workgroups take bursts from the queue, the long ones first, as k_zeros does).  Its rows [restart, stop) are
//   head    kDzHead rows, a lane per track, literally: the staggered start of the tracks (src/decoder.c:855-861), the deskew FIFO
//           filling (a track reads row n while n - restart < delay, row n - delay afterwards), row `restart` differentiated against 0,
//   chunks  of up to kDzThreads / ntrks sub-segments of kDzSub rows (the burst's last one may be shorter): a lane per (sub-segment, track).
//           Pass 1 walks the lane's rows from "none" (its map), a lane per track composes the chunk's maps in order from the track's
//           true state - every lane then knows its entry state and its first event's slot -, pass 2 walks the same rows again (they
//           lie in L2) from that state and stores the events where they belong.
// The arithmetic is the literal float one (volt(), two roundings, dead band, x 0.4f x samples_per_bit; -ffp-contract=off).
// Output: byte for byte what k_decode's walk_diffzeros writes (rtfe_kernels.hip).  Included behind rtfe_kernels.hip.

namespace rtfe {

constexpr int kDzHead = 64;            // rows walked literally at a burst's start (> RTFE_MAXTRKS and > the largest deskew delay, 50)
constexpr int kDzSub = 128;            // rows of a sub-segment
constexpr int kDzThreads = 256;        // lanes of a workgroup: kDzThreads / ntrks sub-segments a chunk
constexpr int kDzLong = 32768;         // bursts of that many rows and more are taken first, those under a quarter of it last
static_assert(kDzHead > RTFE_MAXTRKS && kDzHead > 50, "the head must cover the staggered starts and the deskew FIFO");
enum { kDzNone = 0, kDzUp = 1, kDzDn = 2 };
enum { kDzfCnt, kDzfBits, kDzfFz, kDzfLz, kDzfN };            // a lane's record: pass 1 leaves its map there, the scan its entry state
enum { kDzbPend = 3, kDzbHz = 4, kDzbMerged = 8, kDzbPos = 16, kDzbNeg = 32 };

// rows are counted from the restart row in 32 bits, modulo 2^32 (as event::sample is): only differences are used
struct DzState { unsigned int fz, lz, nev; int pend; bool hz; };      // first / last exact zero since the last arming row or event (hz: there is one)

// the sample's code: -invert negates the voltage, and -(-32768) is +32768 (zc_code)
__device__ __forceinline__ int dz_code(int raw, bool inv) { return inv ? -raw : raw; }
// differentiate() for one sample (src/readtape.c:1383-1388): the float operations of walk_diffzeros
__device__ __forceinline__ float dz_diff(float vraw, float vprev, int spb) {
   float delta = vraw - vprev;
   if (delta < 0.05f && delta > -0.05f) delta = 0;
   return delta * 0.4f * spb; }

struct DzOut { rtfe_event *evp; unsigned int cap; int trk; unsigned int flags; };

__device__ __forceinline__ void dz_event(DzState &s, DzOut &o, float v, unsigned int n, bool up) {
   const unsigned int d1 = s.hz ? n - s.fz : 0u, d2 = s.hz ? n - s.lz : 0u;
   if (s.nev < o.cap && d1 < 65536u) {
      rtfe_event e;
      e.sample = n;
      e.v_peak = v;
      e.agc_gain = __uint_as_float((d1 << 16) | d2);
      e.trk = (uint8_t)o.trk;
      e.flags = (uint8_t)(up ? 0 : 1);
      e.left_distance = (uint8_t)(d1 < 255 ? d1 : 255);
      e.parmset = 0;
      o.evp[s.nev] = e; }
   else o.flags |= RTFE_F_EVENT_OVERFLOW; }

// One row of the detector (the reference's statements in their order).  kEmit: the events are stored; else only counted, and
// `bits` collects kDzbMerged / kDzbPos / kDzbNeg (the head of the file)
template <bool kEmit> __device__ __forceinline__ void dz_step(DzState &s, DzOut &o, unsigned int &bits, float v, unsigned int n) {
   if (v > 0) {
      if (!kEmit && !(bits & kDzbMerged)) bits |= kDzbPos;
      if (s.pend == kDzUp) {
         if (kEmit) dz_event(s, o, v, n, true);
         ++s.nev; s.pend = kDzNone; s.hz = false; }
      if (v > 0.2f) { s.pend = kDzDn; s.hz = false; if (!kEmit) bits |= kDzbMerged; } }
   else if (v < 0) {
      if (!kEmit && !(bits & kDzbMerged)) bits |= kDzbNeg;
      if (s.pend == kDzDn) {
         if (kEmit) dz_event(s, o, v, n, false);
         ++s.nev; s.pend = kDzNone; s.hz = false; }
      if (v < -0.2f) { s.pend = kDzUp; s.hz = false; if (!kEmit) bits |= kDzbMerged; } }
   else { s.lz = n; if (!s.hz) { s.fz = n; s.hz = true; } } }

// A lane's rows behind the head: detector rows n0 .. n0 + len - 1 (relative to the restart: n_rel0) of one track, whose samples are
// p[0], p[P], .. with p[-P] the sample the first one is differentiated against.  Eight loads in flight; no row behind the last is read.
template <bool kEmit> __device__ __forceinline__ void dz_rows(DzState &s, DzOut &o, unsigned int &bits, gptr16 p, int P, int len, unsigned int n_rel0,
                                                              float mv, int spb, bool inv) {
   float vprev = volt(dz_code(p[-P], inv), mv);
   #pragma nounroll
   for (int i = 0; i < len; i += 8) {
      int x8[8];
      #pragma unroll
      for (int k = 0; k < 8; ++k) { const int r = i + k < len ? i + k : len - 1; x8[k] = p[r * P]; }
      #pragma unroll
      for (int k = 0; k < 8; ++k) {
         if (i + k < len) {
            const float vraw = volt(dz_code(x8[k], inv), mv);
            dz_step<kEmit>(s, o, bits, dz_diff(vraw, vprev, spb), n_rel0 + (unsigned int)(i + k));
            vprev = vraw; } } } }

__global__ void __launch_bounds__(kDzThreads) k_diffz(const DevCfg *__restrict__ cfgp, const int16_t *__restrict__ rows, long long nrows, long long row_base,
                                                      rtfe_burst *__restrict__ bursts, BurstScratch *__restrict__ scratch,
                                                      uint32_t *__restrict__ counts, rtfe_event *__restrict__ events) {
   __shared__ DevCfg cfg;
   __shared__ int s_burst;
   __shared__ unsigned int s_flags;
   __shared__ DzState walkers[RTFE_MAXTRKS];
   __shared__ unsigned int rec[kDzfN][kDzThreads];         // the lanes' records, field-major
   for (int i = threadIdx.x; i < (int)(sizeof(DevCfg) / 4); i += blockDim.x) reinterpret_cast<int *>(&cfg)[i] = reinterpret_cast<const int *>(cfgp)[i];
   __syncthreads();
   const int ntrks = cfg.ntrks;
   const int nsub_max = kDzThreads / ntrks;
   const int T = threadIdx.x;
   const bool is_walker = T < ntrks;
   const int j = T / ntrks, t = T - j * ntrks;            // thread -> (sub-segment j, track t), the tracks of a sub-segment side by side: neighbouring lanes read one row's bytes
   const int col = cfg.trk_to_head[t], d = cfg.skew[t];
   const float mv = cfg.maxvolts;
   const int spb = cfg.samples_per_bit;
   const bool inv = cfg.invert != 0;
   for (;;) {
      if (T == 0) { s_burst = atomicAdd(&scratch->queue, 1); s_flags = 0; }
      __syncthreads();
      // the queue is gone through three times: the long bursts first, the short ones last (a burst is one workgroup's from start to end)
      const int nq = scratch->nbursts;
      if (s_burst >= 3 * nq) break;
      const int pass = s_burst / (nq > 0 ? nq : 1), b = s_burst - pass * nq;
      const int nb = scratch->nbursts_total;
      const rtfe_burst B = bursts[b];
      const bool exact = B.flags & RTFE_F_EXACT_START;
      // any restart inside the zone is equivalent for this detector: the zone's last kMarginRows rows
      long long reset = B.reset_sample;
      unsigned int bflags = B.flags;
      if (!exact) {
         reset = B.zone_end - kMarginRows;
         if (B.zone_end - B.zone_first < kMarginRows + 64) bflags |= RTFE_F_UNSAFE; }
      long long stop = nrows;
      if (b + 1 < nb) {
         const rtfe_burst NB = bursts[b + 1];
         stop = NB.zone_end - kMarginRows;
         if (cfg.tail_rows > 0 && NB.zone_first + cfg.tail_rows < stop) stop = NB.zone_first + cfg.tail_rows; }
      if (stop > nrows) stop = nrows;
      const long long len = stop - reset;
      if ((len >= kDzLong ? 0 : (len >= kDzLong / 4 ? 1 : 2)) != pass) { __syncthreads(); continue; }
      DzOut o;
      o.evp = events + B.event_base + (size_t)t * B.event_cap; o.cap = B.event_cap; o.trk = t; o.flags = 0;
      unsigned int nobits = 0;
      // ---- head: the staggered start of the tracks and the filling of the deskew FIFO, row by row ----
      long long c0 = reset + kDzHead < stop ? reset + kDzHead : stop;
      if (is_walker) {
         DzState s; s.fz = 0; s.lz = 0; s.nev = 0; s.pend = kDzNone; s.hz = false;
         const gptr16 x = (gptr16)rows + col;
         for (long long n = reset + T + 1; n < c0; ++n) {            // row restart + T only seeds the track (src/decoder.c:855-861)
            const long long src = (n - reset < d) ? n : n - d;
            const float vraw = volt(dz_code(x[src * ntrks], inv), mv);
            const float vprev = src == reset ? 0.0f : volt(dz_code(x[(src - 1) * ntrks], inv), mv);      // v_last_raw = 0 at the restart (src/decoder.c:437)
            dz_step<true>(s, o, nobits, dz_diff(vraw, vprev, spb), (unsigned int)(n - reset)); }
         walkers[T] = s; }
      __syncthreads();
      // ---- chunks of ns sub-segments ----
      while (c0 < stop) {
         const long long left = (stop - c0 + kDzSub - 1) / kDzSub;
         const int ns = left < nsub_max ? (int)left : nsub_max;
         const bool mine = j < ns;
         const long long n0 = c0 + (long long)j * kDzSub;
         const int mylen = mine ? (int)(stop - n0 < kDzSub ? stop - n0 : kDzSub) : 0;
         const gptr16 p = (gptr16)rows + (mine ? n0 - d : reset) * ntrks + col;
         const unsigned int n_rel0 = (unsigned int)(n0 - reset);
         unsigned int mycnt = 0, mybits = 0;
         if (mine) {
            DzState s; s.fz = 0; s.lz = 0; s.nev = 0; s.pend = kDzNone; s.hz = false;
            dz_rows<false>(s, o, mybits, p, ntrks, mylen, n_rel0, mv, spb, inv);
            mycnt = s.nev;
            rec[kDzfCnt][T] = s.nev; rec[kDzfBits][T] = mybits | (unsigned int)s.pend | (s.hz ? kDzbHz : 0u); rec[kDzfFz][T] = s.fz; rec[kDzfLz][T] = s.lz; }
         __syncthreads();
         // ---- a lane per track composes the maps in order: every lane's entry state and first slot, the track's state behind the chunk ----
         if (is_walker) {
            DzState cur = walkers[T];
            for (int k = 0; k < ns; ++k) {
               const int L = k * ntrks + T;
               const unsigned int cnt = rec[kDzfCnt][L], bits = rec[kDzfBits][L], fz = rec[kDzfFz][L], lz = rec[kDzfLz][L];
               rec[kDzfCnt][L] = cur.nev; rec[kDzfBits][L] = (unsigned int)cur.pend | (cur.hz ? kDzbHz : 0u); rec[kDzfFz][L] = cur.fz; rec[kDzfLz][L] = cur.lz;
               const bool extra = (cur.pend == kDzUp && (bits & kDzbPos)) || (cur.pend == kDzDn && (bits & kDzbNeg));
               cur.nev += cnt + (extra ? 1u : 0u);
               if (bits & kDzbMerged) { cur.pend = (int)(bits & kDzbPend); cur.hz = (bits & kDzbHz) != 0; cur.fz = fz; cur.lz = lz; }
               else if (extra) { cur.pend = kDzNone; cur.hz = false; }
               else if (cur.pend != kDzNone && (bits & kDzbHz)) {       // still pending, nothing reset the zeros: the stretch's join the entry's
                  if (!cur.hz) { cur.fz = fz; cur.hz = true; }
                  cur.lz = lz; } }
            walkers[T] = cur; }
         __syncthreads();
         // ---- pass 2: the lanes that have events walk their rows again, from the true state ----
         if (mine) {
            const unsigned int ebits = rec[kDzfBits][T];
            DzState s; s.nev = rec[kDzfCnt][T]; s.pend = (int)(ebits & kDzbPend); s.hz = (ebits & kDzbHz) != 0; s.fz = rec[kDzfFz][T]; s.lz = rec[kDzfLz][T];
            const bool extra = (s.pend == kDzUp && (mybits & kDzbPos)) || (s.pend == kDzDn && (mybits & kDzbNeg));
            if (mycnt || extra) dz_rows<true>(s, o, nobits, p, ntrks, mylen, n_rel0, mv, spb, inv); }
         c0 += (long long)ns * kDzSub; }
      // ---- publish (as k_decode does for this detector) ----
      if (o.flags) atomicOr(&s_flags, o.flags);
      if (is_walker) {
         const DzState &w = walkers[T];
         if (w.pend != kDzNone) atomicOr(&s_flags, (unsigned int)RTFE_F_STATE_AT_END);      // history a restart would not have
         counts[((size_t)b * cfg.nparm + 0) * ntrks + T] = w.nev < B.event_cap ? w.nev : B.event_cap; }
      for (int i = T; i < (cfg.nparm - 1) * ntrks; i += blockDim.x) counts[((size_t)b * cfg.nparm + 1) * ntrks + i] = 0;      // (the detector does not depend on the parameter set: set 0 only)
      __syncthreads();
      if (T == 0) {
         bursts[b].reset_sample = reset;
         bursts[b].safe_last = (bflags & RTFE_F_UNSAFE) ? -1 : (!exact ? B.zone_end - ntrks - 2 : reset);
         bursts[b].end_sample = stop;
         bursts[b].flags = bflags | s_flags; }
      __syncthreads(); } }

}  // namespace rtfe
