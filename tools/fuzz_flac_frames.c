/* Replays FLAC files through wh_flac_decode_frames (the host twin of the GPU decode, csrc/flac_decode.c + flac_core.h) and
 * through byte-level mutations of them; meant to be built with sanitizers, as a program of its own:
 *   python tools/dump_flac_cases.py DIR
 *   gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/fuzz_flac_frames.c \
 *       whisper_amd/csrc/flac_decode.c -o tools/fuzz_flac_frames && tools/fuzz_flac_frames 300 DIR/*.flac
 * Every unmutated file that wh_flac_decode accepts must come out of the twin with the same samples (or be refused by it);
 * mutations only have to come back. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "whisper_audio.h"
#include "whisper_flac_frames.h"

static uint32_t rs = 12345;
static uint32_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 17; rs ^= rs << 5; return rs; }

static int twin(const unsigned char* d, size_t n, int32_t** pcm, int64_t* ns, int* ch) {
  int rate = 0, bps = 0; int32_t stats[4]; int64_t st[64], en[64]; int32_t bs[64], rc[64];
  return wh_flac_decode_frames(d, n, pcm, ns, ch, &rate, &bps, stats, st, bs, en, rc, 64);
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s MUTATIONS FILE...\n", argv[0]); return 2; }
  const int iters = atoi(argv[1]);
  long same = 0, refused = 0, mut_ok = 0, mut_bad = 0;
  for (int a = 2; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    unsigned char* base = malloc(n ? n : 1);
    if (fread(base, 1, n, f) != (size_t)n) return 2;
    fclose(f);
    int32_t *p0 = NULL, *p1 = NULL; int64_t n0 = 0, n1 = 0; int c0 = 0, c1 = 0, r = 0, b = 0;
    const int rc0 = wh_flac_decode(base, (size_t)n, &p0, &n0, &c0, &r, &b);
    const int rc1 = twin(base, (size_t)n, &p1, &n1, &c1);
    if (rc1 == 0) {
      /* the twin accepts what the host decoder accepts, or what fails the MD5 only */
      if (rc0 == 0 && (n0 != n1 || c0 != c1 || memcmp(p0, p1, (size_t)n0 * c0 * 4))) { printf("MISMATCH %s\n", argv[a]); return 1; }
      if (rc0 != 0 && rc0 != -6) { printf("twin accepted what the decoder refused (%d): %s\n", rc0, argv[a]); return 1; }
      ++same;
    } else ++refused;
    wh_flac_free(p0); wh_flac_free(p1);
    for (int it = 0; it < iters && n > 0; ++it) {
      long len = n;
      unsigned char* d = malloc(n);          /* exactly n bytes: a read past the end is a sanitizer report */
      memcpy(d, base, n);
      const int mode = rnd() % 5;
      if (mode == 0) len = rnd() % n;
      else if (mode == 1) { for (int k = 0; k < 1 + (int)(rnd() % 8); ++k) d[rnd() % n] ^= 1u << (rnd() % 8); }
      else if (mode == 2) { long p = rnd() % n, m = 1 + rnd() % 64; if (p + m > n) m = n - p; for (long k = 0; k < m; ++k) d[p + k] = rnd(); }
      else if (mode == 3) { for (int k = 0; k < 4; ++k) d[rnd() % (n < 64 ? n : 64)] = rnd(); }
      else { long p = rnd() % n; for (int k = 0; k < 16 && p + k < n; ++k) d[p + k] = 0xff; }
      int32_t* pm = NULL; int64_t nm = 0; int cm = 0;
      unsigned char* e = malloc(len ? len : 1); memcpy(e, d, len);     /* tight buffer for the truncated case as well */
      if (twin(e, (size_t)len, &pm, &nm, &cm) == 0) { ++mut_ok; volatile int64_t s = 0; for (int64_t i = 0; i < nm * cm; i += 97) s += pm[i]; wh_flac_free(pm); }
      else ++mut_bad;
      free(e); free(d);
    }
    free(base);
  }
  printf("files: %ld equal to wh_flac_decode, %ld refused by the twin; mutations: %ld decoded, %ld refused\n", same, refused, mut_ok, mut_bad);
  return 0;
}
