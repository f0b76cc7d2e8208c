/* rt_csv.h — CSV ingest (replaces the reference's CSV path, src/readtape.c:1426-1448 and its converter src/csvtbin.c:619-716). */
#ifndef RT_CSV_H
#define RT_CSV_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define RT_CSV_MAXTRKS 19
struct rt_csv_info {
   int      columns;        /* data columns the second title line announces */
   int64_t  rows;           /* sample rows behind the title lines (after subsampling) */
   uint64_t tstart_ns;      /* time of the first used sample */
   uint32_t tdelta_ns;      /* sample period */
   float    maxvolts;       /* full scale for the int16 codes */
};
/* first pass: period, start time, full scale (maxvolts_given = 0: derive it), row count */
int rt_csv_survey(const char *path, int ntrks, float scale, int subsample, float maxvolts_given, struct rt_csv_info *out);
/* ... with the pre-read's length given (rt_csv_survey: a million lines; the line on which it stops is counted but not surveyed) */
int rt_csv_survey_n(const char *path, int ntrks, float scale, int subsample, float maxvolts_given, int64_t preread_rows, struct rt_csv_info *out);
/* the timestamp in front of one line, as the survey reads it (the device path parses two of them on the host: the first and the last surveyed line's) */
double rt_csv_scan_time(const char *line);
/* second pass: rows[n][ntrks] int16 codes, column k of the file going to column perm[k] (NULL = identity); returns the rows written */
int64_t rt_csv_load(const char *path, int ntrks, const int *perm, int invert, float scale, int subsample, float maxvolts,
                    int16_t *rows, int64_t capacity, int64_t *clipped);

/* ---- the converter's window options, -graph and -redo (src/csvtbin.c:364-376, 661-747) ---- */
enum { RT_CSV_ENDED_FILE = 0, RT_CSV_ENDED_STOPAFT = 1, RT_CSV_ENDED_ENDTIME = 2 };      /* how a pass ended */
struct rt_csv_window {
   int64_t skipped;         /* K: raw data lines the skipping loop drops */
   int64_t first_line;      /* the raw data line (0 = the file's third line) of the first sample: K + subsample - 1 */
   int64_t count;           /* samples written; sample j is raw data line first_line + j * subsample */
   int     ended;           /* RT_CSV_ENDED_* */
};
/* the samples that -skip / -starttime / -endtime / -stopaft leave of a file of data_lines raw data lines (a value <= 0: not given); tstart_ns / tdelta_ns
 * are the survey's, after its -subsample adjustment.  -5: the file ends inside the skip */
int rt_csv_convert_window(uint64_t tstart_ns, uint32_t tdelta_ns, int64_t data_lines, int subsample, int64_t skip, float starttime, float endtime,
                          int64_t stopaft, struct rt_csv_window *out);
uint64_t rt_csv_seconds_ns(float seconds);            /* an option's seconds as the converter takes them */
float rt_csv_redo_maxvolts(float newmax);             /* -redo's full scale for the largest magnitude of the first pass */
struct rt_csv_pass_opts {
   int ntrks; const int *perm; int invert; float scale; int subsample; float maxvolts;
   int64_t skip; float starttime, endtime; int64_t stopaft; int64_t graphbin;      /* <= 0: not given */
   uint64_t tstart_ns; uint32_t tdelta_ns;
};
struct rt_csv_pass {
   int64_t skipped, samples, too_big, too_small, graph_lines;
   int     ended;           /* RT_CSV_ENDED_* */
   float   newmax;          /* the largest |sample| in volts: what -redo sizes the second pass by */
};
/* one pass over the file into whatever sinks are given (NULL: not wanted): rows in memory, a .tbin file, a graph file, the graph as numbers */
int rt_csv_convert_pass(const char *csv_path, const struct rt_csv_pass_opts *o, int16_t *rows, int64_t capacity, const char *tbin_path, const void *header,
                        int header_bytes, const char *graph_path, int64_t *graph_at, float *graph_max, int64_t graph_cap, struct rt_csv_pass *res);
/* "<(i + 1) * graphbin>, <%f of bins[i]>" per bin: the graph file from maxima made elsewhere (rtfe_csv_graph) */
int rt_csv_graph_write(const char *graph_path, int64_t graphbin, const float *bins, int64_t nbins);

/* ---- the other direction: rows -> the text of the converter's -read (src/csvtbin.c:523-596; rt_csvout.c) ---- */
/* the rows [*first, *first + *count) that -skip / -starttime / -endtime / -stopaft leave of nrows rows (a value <= 0: not given) */
int rt_csv_export_window(uint64_t tstart_ns, uint32_t tdelta_ns, int64_t nrows, int64_t skip, float starttime, float endtime, int64_t stopaft,
                         int64_t *first, int64_t *count);
/* the two title lines and those rows, by fprintf; column k prints rows[.][perm ? perm[k] : k].  Returns the bytes written, negative on failure */
int64_t rt_csv_export_write(const char *path, const char *descr, int ntrks, const int *perm, int invert, float maxvolts, float stagger,
                            uint64_t tstart_ns, uint32_t tdelta_ns, const int16_t *rows, int64_t first, int64_t count);
#ifdef __cplusplus
}
#endif
#endif
