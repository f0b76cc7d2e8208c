/* csvconv_asan_main.c — the window rule and the host writer of the CSV -> TBIN conversion (csrc/host/rt_csv.c) in a program of their own, for a
 * sanitizer run on the CPU:
 *
 *   gcc -std=gnu99 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -D_DEFAULT_SOURCE -Ireadtape_amd/csrc/host \
 *       -o csvconv_asan tests/csvconv_asan_main.c readtape_amd/csrc/host/rt_csv.c readtape_amd/csrc/host/rt_csvout.c -lm
 *   ./csvconv_asan <a directory to write into>
 *
 * It writes a CSV of a few thousand lines (short lines, a blank one, one longer than the line buffer, no newline at the end), converts it with every
 * combination of a few window options into memory, into files and into both, checks each pass against rt_csv_convert_window, and prints "ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt_csv.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

enum { NLINES = 3000, NTRKS = 7 };

static int64_t file_size(const char *path) {
   FILE *f = fopen(path, "rb");
   if (!f) return -1;
   fseek(f, 0, SEEK_END);
   const int64_t n = ftell(f);
   fclose(f);
   return n; }

int main(int argc, char **argv) {
   CHECK(argc == 2);
   char csv[600], out[600], graph[600];
   snprintf(csv, sizeof csv, "%s/asan.csv", argv[1]);
   snprintf(out, sizeof out, "%s/asan.tbin", argv[1]);
   snprintf(graph, sizeof graph, "%s/asan.graph.csv", argv[1]);
   FILE *f = fopen(csv, "w");
   CHECK(f);
   fprintf(f, "export\nTime [s], a, b, c, d, e, f, g\n");
   uint32_t r = 12345;
   for (int i = 0; i < NLINES; ++i) {
      fprintf(f, "%.7f", 0.0125 + i * 2e-6);
      const int fields = i == 700 ? 2 : NTRKS;                               /* a short line */
      for (int k = 0; k < fields; ++k) {
         r = r * 1664525u + 1013904223u;
         double v = ((int)(r >> 8) % 60000) / 10000.0 - 3.0;
         if (i > 2500 && k == 3) v *= 4;                                     /* clips behind the pre-read */
         fprintf(f, ", %.4f", v); }
      if (i == 900) for (int k = 0; k < 500; ++k) fputc(' ', f);              /* longer than fgets(line, 400) returns whole: two lines to the reader */
      if (i == 1200) fputc('\n', f);                                        /* a blank line */
      if (i != NLINES - 1) fputc('\n', f); }
   fclose(f);

   struct rt_csv_info info;
   CHECK(rt_csv_survey_n(csv, NTRKS, 1.0f, 1, 0.0f, 2000, &info) == 0);
   const int64_t lines = info.rows;                                          /* raw data lines, as fgets counts them */
   CHECK(lines == NLINES + 2 && info.columns == NTRKS);
   int perm[NTRKS] = { 5, 4, 3, 2, 1, 0, 6 };
   int16_t *rows = (int16_t *)malloc(sizeof(int16_t) * NTRKS * (size_t)lines);
   int64_t *g_at = (int64_t *)malloc(sizeof(int64_t) * (size_t)lines);
   float *g_max = (float *)malloc(sizeof(float) * (size_t)lines);
   CHECK(rows && g_at && g_max);
   const int64_t skips[] = { 0, 1, 17, lines, lines + 1 }, stops[] = { 0, 1, 64, 100000 }, bins[] = { 0, 1, 64, 100000 };
   const float starts[] = { 0.0f, 0.01f, 0.0126f, 0.5f }, ends[] = { 0.0f, 0.0127f, 0.9f };
   int passes = 0;
   for (int sub = 1; sub <= 3; ++sub) for (unsigned a = 0; a < 5; ++a) for (unsigned b = 0; b < 4; ++b) for (unsigned c = 0; c < 4; ++c) for (unsigned d = 0; d < 3; ++d)
   for (unsigned e = 0; e < 4; ++e) {
      struct rt_csv_info s;
      CHECK(rt_csv_survey_n(csv, NTRKS, 0.5f, sub, 0.0f, 2000, &s) == 0);
      struct rt_csv_pass_opts o = { NTRKS, (a & 1) ? perm : NULL, (int)(b & 1), 0.5f, sub, s.maxvolts, skips[a], starts[c], ends[d], stops[b], bins[e], s.tstart_ns, s.tdelta_ns };
      struct rt_csv_window w;
      const int wrc = rt_csv_convert_window(s.tstart_ns, s.tdelta_ns, lines, sub, skips[a], starts[c], ends[d], stops[b], &w);
      struct rt_csv_pass res;
      const int sinks = (int)((a + b + c + d + e) % 3);                      /* memory, files, both */
      const int rc = rt_csv_convert_pass(csv, &o, sinks != 1 ? rows : NULL, lines, sinks != 0 ? out : NULL, "HEAD", 4, sinks != 0 ? graph : NULL,
                                         g_at, g_max, lines, &res);
      ++passes;
      if (wrc == -5) { CHECK(rc == -5); continue; }
      CHECK(wrc == 0 && rc == 0);
      CHECK(res.skipped == w.skipped && res.samples == w.count && res.ended == w.ended);
      const int64_t glines = bins[e] > 0 && w.count > 0 ? (w.ended == RT_CSV_ENDED_FILE ? w.count : w.count - 1) / bins[e] : 0;
      CHECK(res.graph_lines == glines);
      for (int64_t i = 0; i < glines; ++i) CHECK(g_at[i] == (i + 1) * bins[e] && g_max[i] >= 0);
      if (sinks != 0) {
         CHECK(file_size(out) == 4 + 2 * NTRKS * w.count + 2);
         if (bins[e] > 0) { CHECK(rt_csv_graph_write(graph, bins[e], g_max, glines) == 0); CHECK((file_size(graph) > 0) == (glines > 0)); } }
      if (res.too_big + res.too_small) CHECK(rt_csv_redo_maxvolts(res.newmax) > s.maxvolts); }
   /* refusals touch nothing */
   struct rt_csv_pass res;
   struct rt_csv_pass_opts o = { 0, NULL, 0, 1.0f, 1, 5.0f, 0, 0, 0, 0, 0, 0, 1000 };
   CHECK(rt_csv_convert_pass(csv, &o, rows, lines, NULL, NULL, 0, NULL, NULL, NULL, 0, &res) == -3);
   o.ntrks = NTRKS; perm[2] = 9; o.perm = perm;
   CHECK(rt_csv_convert_pass(csv, &o, rows, lines, NULL, NULL, 0, NULL, NULL, NULL, 0, &res) == -4);
   o.perm = NULL;
   CHECK(rt_csv_convert_pass(csv, &o, rows, 10, NULL, NULL, 0, NULL, NULL, NULL, 0, &res) == -8);
   CHECK(rt_csv_convert_pass("/nonexistent/x.csv", &o, rows, lines, NULL, NULL, 0, NULL, NULL, NULL, 0, &res) == -1);
   free(rows); free(g_at); free(g_max);
   printf("ok: %d passes\n", passes);
   return 0; }
