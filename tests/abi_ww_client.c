/* A plain-C caller of the Whirlwind detector entry points (include/rt_frontend.h): makes a -differentiate -zeros handle, asks it for its
 * state kind and size, makes the initial state, uploads a flat tape and scans it once.  Prints "ok <kind> <bytes> <events>".
 * TEST INFRASTRUCTURE (tests/test_gpu_ww_detectors.py builds it with gcc -std=gnu99 and runs it on the GPU). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime_api.h>
#include "rt_frontend.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP call failed at line %d\n", __LINE__); return 3; } } while (0)

int main(void) {
   rtfe_config c;
   memset(&c, 0, sizeof c);
   c.mode = RTFE_WW; c.ntrks = 6; c.maxvolts = 4.4f; c.bpi = 100.0f; c.ips = 50.0f; c.tdelta_ns = 5000; c.nparmsets = 1;
   for (int i = 0; i < 6; ++i) c.head_to_trk[i] = i;
   c.parmset[0].pkww_bitfrac = 0.7f; c.parmset[0].pkww_rise = 0.1f; c.parmset[0].agc_alpha = 0.3f;
   c.find_zeros = 1; c.differentiate = 1;
   rtfe_handle *h = NULL;
   if (rtfe_create(&c, &h) != 0) { fprintf(stderr, "rtfe_create: %s\n", rtfe_last_error()); return 1; }
   const int kind = rtfe_ww_state_kind(h);
   const size_t per_track = rtfe_ww_state_bytes(h), sbytes = per_track * 6;
   if (kind != RTFE_WW_DIFFZEROS || per_track != sizeof(rtfe_ww_dtrack)) { fprintf(stderr, "kind %d, %zu bytes a track\n", kind, per_track); return 1; }
   rtfe_ww_dtrack st[6];
   if (rtfe_ww_detector_initial_state(h, st, sbytes - 1) == 0) { fprintf(stderr, "a short state buffer was accepted\n"); return 1; }
   if (rtfe_ww_detector_initial_state(h, st, sbytes) != 0) { fprintf(stderr, "initial state: %s\n", rtfe_last_error()); return 1; }
   enum { NROWS = 2048, CAP = 2048 };
   int16_t *rows = (int16_t *)calloc((size_t)NROWS * 6, sizeof(int16_t));
   for (int n = 0; n < NROWS; ++n) rows[n * 6 + 1] = (int16_t)(((n / 40) & 1) ? 9000 : -9000);      /* a square wave on track 1 */
   void *d_rows, *d_in, *d_out, *d_counts, *d_events, *d_flags;
   CHECK(hipMalloc(&d_rows, (size_t)NROWS * 12)); CHECK(hipMalloc(&d_in, sbytes)); CHECK(hipMalloc(&d_out, sbytes));
   CHECK(hipMalloc(&d_counts, 6 * 4)); CHECK(hipMalloc(&d_events, (size_t)6 * CAP * sizeof(rtfe_ww_event))); CHECK(hipMalloc(&d_flags, 4));
   CHECK(hipMemcpy(d_rows, rows, (size_t)NROWS * 12, hipMemcpyHostToDevice)); CHECK(hipMemcpy(d_in, st, sbytes, hipMemcpyHostToDevice));
   CHECK(hipMemset(d_flags, 0, 4));
   if (rtfe_ww_detector_scan(h, (const int16_t *)d_rows, NROWS, 0, 0, NROWS, 0, d_in, d_out, sbytes - 8, (uint32_t *)d_counts, (rtfe_ww_event *)d_events, CAP,
                             (uint32_t *)d_flags, NULL) == 0) { fprintf(stderr, "a state buffer of the wrong size was accepted\n"); return 1; }
   if (rtfe_ww_detector_scan(h, (const int16_t *)d_rows, NROWS, 0, 0, NROWS, 0, d_in, d_out, sbytes, (uint32_t *)d_counts, (rtfe_ww_event *)d_events, CAP,
                             (uint32_t *)d_flags, NULL) != 0) { fprintf(stderr, "scan: %s\n", rtfe_last_error()); return 1; }
   CHECK(hipDeviceSynchronize());
   uint32_t counts[6], flags = 0;
   CHECK(hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(&flags, d_flags, 4, hipMemcpyDeviceToHost));
   CHECK(hipMemcpy(st, d_out, sbytes, hipMemcpyDeviceToHost));
   if (flags != 0 || st[1].kind != RTFE_WW_DIFFZEROS || st[1].v_last_raw != rows[(NROWS - 1) * 6 + 1]) { fprintf(stderr, "flags %u kind %d last raw %d\n", flags, st[1].kind, st[1].v_last_raw); return 1; }
   printf("ok %d %zu %u\n", kind, per_track, counts[1]);
   rtfe_destroy(h);
   return 0; }
