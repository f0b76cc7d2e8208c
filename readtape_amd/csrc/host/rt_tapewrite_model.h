/* rt_tapewrite_model.h — the tape writer's waveform model as code: the few expressions that decide a sample's bytes, in one place, compiled into the host
 * renderer (rt_tapewrite.c, gcc) and into the kernel (rtfe_tapewrite.hip, hipcc: RT_TW_FN is defined there).  The model in words: include/rt_frontend.h,
 * rtfe_tape_render.  It is readtape_amd/synth.py's (_render_block, _render_pulses, _quantise), every expression in that file's operation order; both builds
 * pass -ffp-contract=off, so a + b * c is two roundings on either side.  Only integer operations and IEEE double + - * / rint: no libm function whose last
 * place could differ between the two.  What walks the slots and the rows is NOT here: the host goes pulse by pulse, the kernel sample by sample. */
#ifndef RT_TAPEWRITE_MODEL_H
#define RT_TAPEWRITE_MODEL_H
#include <math.h>
#include <stdint.h>

#include "rt_frontend.h"

#ifndef RT_TW_FN
#define RT_TW_FN static inline
#endif

#define RT_TW_LEAD 8.0                       /* cells of nothing in front of and behind a block's cells (synth._render_block's lead_cells) */
#define RT_TW_GOLDEN 0x9E3779B97F4A7C15ull
#define RT_TW_GMAX 3.4641                    /* |g| <= 131070 * 0x1.bb67ae86627e8p-16 = 3.46404... */

/* the splitmix64 finaliser */
RT_TW_FN uint64_t rt_tw_mix(uint64_t z) {
   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
   z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
   return z ^ (z >> 31); }

/* g(key, n): the sum of four uniform 16-bit fields, centred, over its standard deviation sqrt((65536^2 - 1) / 3) = 37837.2272... */
RT_TW_FN double rt_tw_gauss(uint64_t key, uint64_t n) {
   const uint64_t z = rt_tw_mix(key + n * RT_TW_GOLDEN);
   const int64_t s = (int64_t)((z & 0xffffu) + ((z >> 16) & 0xffffu) + ((z >> 32) & 0xffffu) + (z >> 48));
   return (double)(s - 131070) * 0x1.bb67ae86627e8p-16; }

/* where the transition of track t in slot s of a block is centred, in rows from the block's first; abs_slot: the slot's index in the whole stream */
RT_TW_FN double rt_tw_centre(double spb, int pitch_shift, double skew, double jitter, uint64_t jkey, int64_t s, int64_t abs_slot) {
   const double cell = (double)s * (pitch_shift ? 0.5 : 1.0);
   const double jit = jitter > 0 ? rt_tw_gauss(jkey, (uint64_t)abs_slot) * jitter : 0.0;
   return (RT_TW_LEAD + cell + 0.5 + skew + jit) * spb; }

/* what a pulse of signed amplitude a centred at c adds to row r */
RT_TW_FN double rt_tw_pulse(double a, int64_t r, double c, double w, double edge) {
   const double d = ((double)r - c) / w;
   return a * (1.0 / (1.0 + d * d) - edge); }

/* the noise of track key's row */
RT_TW_FN double rt_tw_noise(double noise_mv, uint64_t nkey, int64_t row) {
   return noise_mv > 0 ? rt_tw_gauss(nkey, (uint64_t)row) * noise_mv * 1e-3 : 0.0; }

RT_TW_FN int16_t rt_tw_quantise(double v, double maxvolts) {
   double q = rint(v / maxvolts * 32767.0);
   if (q > 32767.0) q = 32767.0;
   if (q < -32767.0) q = -32767.0;
   return (int16_t)q; }
#endif
