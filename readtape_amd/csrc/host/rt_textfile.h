/* rt_textfile.h — the interpreted text dump of a tape (src/textfile.c) and the SIMH .tap reader in front of it (src/tapread.c). */
#ifndef RT_TEXTFILE_H
#define RT_TEXTFILE_H
#include <stddef.h>
#include <stdint.h>

#include "rt_text_tables.h"

struct rt_textfile;

/* "<base>.<num>.<char>.txt" (src/textfile.c:192-196); o resolved or not */
int  rt_text_name(const char *base, const rt_text_options *o, char *out, size_t outlen);

/* A writer for <base>'s text file.  tapread: the terse layout of -tapread (and " -tapread" in the title), otherwise the decode
 * path's verbose one.  created: what stands behind "on " in the title's second line, ctime's format with its newline (NULL:
 * the time now).  The file is made when the first thing is written to it, as the reference makes it, or by rt_text_open_now.
 * NULL: the options are out of range. */
struct rt_textfile *rt_text_new(const char *base, const rt_text_options *o, int tapread, const char *created);
int  rt_text_open_now(struct rt_textfile *t);                      /* 0, or -1: the file cannot be made */
void rt_text_message(struct rt_textfile *t, const char *msg);
void rt_text_tapemark(struct rt_textfile *t, double timenow);
/* a record's data bytes; head: the verbose layout's "block N: L bytes at time T, <errors>" (without its line end) */
void rt_text_record(struct rt_textfile *t, const unsigned char *bytes, int length, int errs, int warnings, const char *head);
void rt_text_body(struct rt_textfile *t, const void *text, size_t n);      /* body text made elsewhere (the device): written as it is */
void rt_text_count(struct rt_textfile *t, int length, int errs, int warnings);   /* ... and the record counted for the trailer */
void rt_text_count_items(struct rt_textfile *t, const rt_tap_item *items, int64_t n);   /* ... a table's records and tape marks */
const char *rt_text_filename(const struct rt_textfile *t);
long long rt_text_close(struct rt_textfile *t, int trailer);      /* -> the file's bytes (0: never made), -1: a write failed; frees t */

/* ---- the .tap image ---- */
enum { RT_TAP_OK = 0, RT_TAP_EOF_TOO_SOON = 1, RT_TAP_BAD_MARKER = 2, RT_TAP_BAD_LENGTH = 3, RT_TAP_TOO_BIG = 4, RT_TAP_NO_TRAILING_LENGTH = 5 };
/* The items of an image, in order, into out[0 .. cap) -> how many there are (more than cap: come back with that many).
 * *status: RT_TAP_OK, or why the reference stops with a fatal error behind the last item returned; err: its message. */
int64_t rt_tap_items(const unsigned char *img, uint64_t nbytes, rt_tap_item *out, int64_t cap, int *status, char *err, size_t errlen);
/* -tapread: <base>'s text file of an image.  -> the file's bytes, or -1 (cannot write) / -2 (bad options); *status / err as
 * above - on a fatal error the file holds what the reference had written when it exited (no trailer). */
long long rt_tapread_write(const unsigned char *img, uint64_t nbytes, const char *base, const rt_text_options *o, const char *created,
                           int *status, char *err, size_t errlen);
#endif
