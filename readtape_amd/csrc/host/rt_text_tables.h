/* rt_text_tables.h — the interpreted text dump's options and its thirteen character codes (src/textfile.c:90-176), as data.
 * One header for the host writer (rt_textfile.c), the .tap reader (rt_tapread.c) and the device formatter (../rtfe_textfile.hip,
 * which receives the table of the code in use as a kernel argument and keeps it in LDS). */
#ifndef RT_TEXT_TABLES_H
#define RT_TEXT_TABLES_H
#include <stdint.h>

#define RT_TEXT_VERSION "3.18"          /* the reference version whose text this is (src/readtape.c:362) */
#define RT_TEXT_MAXLINE 400             /* -linesize / -dataspace at most (src/decoder.h:95) */
#define RT_TEXT_MAXBLOCK 131072         /* a record is shorter than this (src/decoder.h:91) */

enum rt_text_num { RT_NUM_NONE, RT_NUM_HEX, RT_NUM_OCTAL, RT_NUM_OCTAL2 };                    /* src/decoder.h:460 */
enum rt_text_char { RT_CHAR_NONE, RT_CHAR_BCD, RT_CHAR_EBCDIC, RT_CHAR_ASCII, RT_CHAR_B5500, RT_CHAR_SIXBIT, RT_CHAR_SDS, RT_CHAR_SDSM,
                    RT_CHAR_FLEXO, RT_CHAR_ADAGE, RT_CHAR_ADAGETAPE, RT_CHAR_CDC, RT_CHAR_UNIVAC, RT_CHAR_COUNT };   /* src/decoder.h:461 */

/* the option names as the title line and the file name spell them (the file name drops the '-') */
static const char *const rt_text_num_names[4] = { " ", "-hex", "-octal", "-octal2" };
static const char *const rt_text_char_names[RT_CHAR_COUNT] = { " ", "-BCD", "-EBCDIC", "-ASCII", "-B5500", "-sixbit", "-SDS", "-SDSM", "-flexo",
                                                               "-adage", "-adagetape", "-CDC", "-Univac" };

/* what a caller asks for; linesize 0 = the default (32 with numbers and characters, otherwise 64), dataspace -1 = the default
 * (2 under octal2, otherwise 0) */
typedef struct rt_text_options {
   int numtype, chartype;
   int linesize, dataspace;
   int linefeed;
   int ntrks;                           /* octal digits a byte: 2 up to 7 tracks, otherwise 3 */
} rt_text_options;

/* an item of a .tap image (rt_tap_items): kind, where its data bytes lie in the image, how many, and its flag
 * (a record: 1 = the marker's error bit; a message: which one) */
enum { RT_TAP_RECORD = 0, RT_TAP_MARK = 1, RT_TAP_MESSAGE = 2 };
enum { RT_TAP_MSG_NO_END = 0, RT_TAP_MSG_ERASED_GAP = 1 };
typedef struct rt_tap_item { uint64_t offset; uint32_t length; uint16_t kind, flag; } rt_tap_item;      /* 16 bytes */

static const char *const rt_tap_messages[2] = { "missing .tap end-of-medium marker\n", "erased gap\n" };
#define RT_TAP_MARK_TEXT "tape mark\n"

/* the 6-bit codes, 64 characters each; lower-case letters stand for symbols ASCII lacks (src/textfile.c:108-155 says which) */
static const char rt_text_code6[RT_CHAR_COUNT][65] = {
   "", /* BCD, IBM 1401 */
   " 1234567890#@:>t" " /STUVWXYZr,%='\"" "-JKLMNOPQR!$*);d" "&ABCDEFGHI?.?(<g",
   "", "",
   /* Burroughs B5500 internal code */
   "0123456789#@?:>}" "+ABCDEFGHI.[&(<~" "|JKLMNOPQR$*-);{" " /STUVWXYZ,%!]=\"",
   "",
   /* SDS internal code */
   "01234567890=':>s" "+ABCDEFGHI?.)[<g" "-JKLMNOPQR!$*];d" " /STUVWXYZr,(~\\#",
   /* SDS magnetic tape code */
   "01234567890#@:>s" " /STUVWXYZt,%~\\g" "-JKLMNOPQRc$*];d" "&ABCDEFGHIb.l[<r",
   /* Flexowriter */
   "  e8 |a3 =s4i+u2" "..d5rlj7n,f6c-k " "t z.l.w h.y p q " "o.b g 9 m.x v.0 ",
   /* Adage AGT */
   " %c!&*:_+t?\"'r()" "0123456789;=,-./" " ABCDEFGHIJKLMNO" "PQRSTUVWXYZ$#@+b",
   /* Adage AGT magnetic tape */
   " 0123456789\"    " "ABCDEFGHOPQRSTUV" "WXYZu@%]IJKLMN  " "+-*/.(),=&: $# r",
   /* CDC 7-track */
   " ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789+-*/()$= ,.#[]:\"_!&'?<>@\\^;",
   /* Univac 7-track */
   "@[]#^ ABCDEFGHIJKLMNOPQRSTUVWXYZ)-+<=>&$*(%:?!,\\0123456789';/.o~" };

/* EBCDIC: the rows 0x40 .. 0xff (everything below 0x40 prints as a blank) */
static const char rt_text_ebcdic[12][17] = {
   "          [.<(+|", "&         !$*);^", "-/        |,%_>?", "         `:#|'=\"",
   " abcdefghi      ", " jklmnopqr      ", " ~stuvwxyz      ", "                ",
   "{ABCDEFGHI      ", "}JKLMNOPQR      ", "\\ STUVWXYZ      ", "0123456789      " };

/* t[odd * 256 + byte]: the character a data byte prints as, at an even / odd index of its record.  Only the Flexowriter code
 * tells the two apart: a 16-bit word holds two 6-bit characters, the high one in the even byte's bits 7..2 */
static inline void rt_text_char_table(int chartype, unsigned char t[512]) {
   for (int odd = 0; odd < 2; ++odd)
      for (int b = 0; b < 256; ++b) {
         unsigned char c = '?';
         switch (chartype) {
         case RT_CHAR_EBCDIC: c = b < 0x40 ? ' ' : (unsigned char)rt_text_ebcdic[(b >> 4) - 4][b & 15]; break;
         case RT_CHAR_ASCII:  c = (b & 0x7f) >= 0x20 && (b & 0x7f) < 0x7f ? (unsigned char)(b & 0x7f) : ' '; break;
         case RT_CHAR_SIXBIT: c = (unsigned char)((b & 0x3f) + 32); break;
         case RT_CHAR_FLEXO:  c = (unsigned char)rt_text_code6[chartype][(odd ? b : b >> 2) & 0x3f]; break;
         case RT_CHAR_BCD: case RT_CHAR_B5500: case RT_CHAR_SDS: case RT_CHAR_SDSM: case RT_CHAR_ADAGE: case RT_CHAR_ADAGETAPE:
         case RT_CHAR_CDC: case RT_CHAR_UNIVAC: c = (unsigned char)rt_text_code6[chartype][b & 0x3f]; break;
         default: break; }
         t[odd * 256 + b] = c; } }

/* the defaults filled in and the ranges checked: 0, or the number of the field that is out of range */
static inline int rt_text_resolve(const rt_text_options *in, rt_text_options *o) {
   *o = *in;
   if (o->numtype < 0 || o->numtype > RT_NUM_OCTAL2) return 1;
   if (o->chartype < 0 || o->chartype >= RT_CHAR_COUNT) return 2;
   if (o->linesize == 0) o->linesize = o->numtype != RT_NUM_NONE && o->chartype != RT_CHAR_NONE ? 32 : 64;
   if (o->linesize < 4 || o->linesize > RT_TEXT_MAXLINE) return 3;
   if (o->dataspace < 0) o->dataspace = o->numtype == RT_NUM_OCTAL2 ? 2 : 0;
   if (o->dataspace > RT_TEXT_MAXLINE) return 4;
   o->linefeed = o->linefeed != 0;
   if (o->ntrks <= 0) o->ntrks = 9;
   return 0; }

#endif
