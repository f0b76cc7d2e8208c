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
