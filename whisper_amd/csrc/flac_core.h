/*
 * flac_core.h — the per-frame FLAC logic (RFC 9639), written once and compiled twice: as plain C into
 * libwhisper_audio.so (flac_decode.c: wh_flac_decode and its frame-parallel twin wh_flac_decode_frames) and as
 * __device__ code into libwhisper_hip.so (flac.hip: one lane per frame).  Bit reader, CRC-8 / CRC-16, frame header,
 * partitioned Rice residuals, CONSTANT / VERBATIM / FIXED / LPC subframes, wasted bits, stereo decorrelation, and the
 * host-side walk that chains independently decoded frames back into a stream.
 *
 * The file has two parts.  The first (include guard) is type independent.  The second is a template over the sample
 * storage type: define FLAC_T and FLAC_SUFFIX, include the file, and get flac_frame<SUFFIX>() and its helpers.
 *   FLAC_T int64_t  "wide":   what wh_flac_decode has always computed in (33-bit side channel of 32-bit audio included)
 *   FLAC_T int32_t  "narrow": the frame-parallel routes, bits per sample <= 24.  Every value is computed in 64 bits from
 *                   sign-extended stored values and checked when it is stored: one that does not survive the narrowing
 *                   sets *range, and the frame is refused (FLAC_E_RANGE).  Without that flag every stored value equals
 *                   the wide one, by induction over the stores, so the narrow result is the wide result.
 *
 * Safe on arbitrary bytes (the frame-parallel routes parse false sync candidates as a matter of course):
 *   - reads past `size` return zero bits; `eof` is set once a read starts 8 bytes past the end (the refill look-ahead);
 *   - every loop runs to a count taken from the frame header: block size <= 65535, channels <= 8, predictor order <= 32,
 *     partitions <= 2^15; a unary run ends with the remaining bits;
 *   - a frame stores to s[c * chan_off + i * stride] with c < channels and i < block size only, and the block size is
 *     refused above the caller's `bs_limit` before the first store;
 *   - arithmetic is unsigned and wrapping; shifts stay below the operand width.
 */
#ifndef WH_FLAC_CORE_H
#define WH_FLAC_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FLAC_FN __host__ __device__ static inline
#else
#define FLAC_FN static inline
#endif

enum { FLAC_OK = 0, FLAC_E_MAGIC = -1, FLAC_E_TRUNC = -2, FLAC_E_HEADER = -3, FLAC_E_CRC = -4, FLAC_E_UNSUP = -5,
       FLAC_E_MD5 = -6, FLAC_E_MEM = -7, FLAC_E_SYNC = -8,
       FLAC_E_RANGE = -9,      /* narrow storage: a value does not fit int32 (frame-parallel routes only) */
       FLAC_E_REJECT = -10 };  /* frame-parallel routes: the stream fails its checks (CRC, chain, sample count) */

enum { FLAC_MAX_BLOCK = 65535, FLAC_MAX_CHANNELS = 8, FLAC_TAIL = 128 /* trailing bytes a stream may carry */ };

/* ---------------------------------------------------------------- bit reader (MSB first) */
typedef struct { const uint8_t* p; size_t n, pos; uint64_t acc; int bits; int eof; } BR;

FLAC_FN void br_init(BR* b, const uint8_t* p, size_t n, size_t pos) { b->p = p; b->n = n; b->pos = pos; b->acc = 0; b->bits = 0; b->eof = 0; }
FLAC_FN void br_fill(BR* b) {
  while (b->bits <= 56) {
    uint64_t byte = 0;
    if (b->pos < b->n) byte = b->p[b->pos];
    else if (b->pos >= b->n + 8) { b->eof = 1; }
    b->pos++;
    b->acc |= byte << (56 - b->bits);
    b->bits += 8;
  }
}
FLAC_FN uint32_t br_u(BR* b, int n) {            /* n in 0..32 */
  if (n == 0) return 0;
  if (b->bits < n) br_fill(b);
  uint32_t v = (uint32_t)(b->acc >> (64 - n));
  b->acc <<= n; b->bits -= n;                      /* n <= 32 */
  return v;
}
FLAC_FN int32_t br_s(BR* b, int n) {             /* signed, n in 1..32 */
  uint32_t v = br_u(b, n);
  if (n < 32 && (v >> (n - 1))) v |= ~0u << n;
  return (int32_t)v;
}
FLAC_FN int64_t br_s64(BR* b, int n) {           /* signed up to 33 bits (side channel of 32-bit audio) */
  if (n <= 32) return br_s(b, n);
  uint64_t hi = (uint64_t)(int64_t)br_s(b, n - 32);
  return (int64_t)((hi << 32) | br_u(b, 32));
}
FLAC_FN uint32_t br_unary(BR* b) {               /* number of 0 bits before the next 1 bit; ends with the stream */
  uint32_t q = 0;
  for (;;) {
    if (b->bits == 0) br_fill(b);
    if (b->acc == 0) { q += (uint32_t)b->bits; b->bits = 0; if (b->eof) return q; continue; }
    int z = __builtin_clzll(b->acc);
    if (z >= b->bits) { q += (uint32_t)b->bits; b->acc = 0; b->bits = 0; continue; }
    q += (uint32_t)z;
    b->acc = z == 63 ? 0 : b->acc << (z + 1);      /* a 64-bit shift would be undefined */
    b->bits -= z + 1;
    return q;
  }
}
FLAC_FN size_t br_bytepos(const BR* b) { return b->pos - (size_t)(b->bits / 8); }   /* valid when byte aligned */
FLAC_FN void br_align(BR* b) { int r = b->bits & 7; b->acc <<= r; b->bits -= r; }

/* ---------------------------------------------------------------- CRCs */
FLAC_FN uint8_t flac_crc8(const uint8_t* p, size_t n) {
  uint8_t c = 0;
  for (size_t i = 0; i < n; ++i) { c ^= p[i]; for (int k = 0; k < 8; ++k) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : c << 1); }
  return c;
}
FLAC_FN uint16_t flac_crc16(const uint8_t* p, size_t n) {
  uint16_t c = 0;
  for (size_t i = 0; i < n; ++i) { c ^= (uint16_t)(p[i] << 8); for (int k = 0; k < 8; ++k) c = (uint16_t)((c & 0x8000) ? (c << 1) ^ 0x8005 : c << 1); }
  return c;
}

/* ---------------------------------------------------------------- frame header */
typedef struct { int blocksize, ch_code, nch; } flac_hdr;

FLAC_FN int flac_is_sync(const uint8_t* data, size_t size, size_t pos) {
  return pos + 2 <= size && data[pos] == 0xFF && (data[pos + 1] & 0xFE) == 0xF8;
}

/* The frame header at `pos` (the caller has seen the sync code there) of a stream of `ch` channels and `bps` bits per
 * sample: FLAC_OK with *h filled and `b` standing behind the CRC-8 byte, or the error wh_flac_decode reports for it. */
FLAC_FN int flac_frame_header(BR* b, const uint8_t* data, size_t size, size_t pos, int ch, int bps, flac_hdr* h) {
  br_init(b, data, size, pos);
  br_u(b, 15);
  br_u(b, 1);                                      /* blocking strategy: the coded number is not used */
  int bs_code = (int)br_u(b, 4), sr_code = (int)br_u(b, 4), ch_code = (int)br_u(b, 4), ss_code = (int)br_u(b, 3);
  if (br_u(b, 1)) return FLAC_E_HEADER;
  /* UTF-8 style coded frame / sample number */
  uint32_t first = br_u(b, 8);
  int ones = 0, extra = 0, bad = 0;
  while (ones < 8 && (first & (0x80u >> ones))) ++ones;
  if (ones == 1 || ones == 8) return FLAC_E_HEADER;
  if (ones) extra = ones - 1;
  for (int i = 0; i < extra; ++i) if ((br_u(b, 8) & 0xC0) != 0x80) bad = 1;
  if (bad) return FLAC_E_HEADER;
  int blocksize;
  if (bs_code == 0) return FLAC_E_HEADER;
  else if (bs_code == 1) blocksize = 192;
  else if (bs_code <= 5) blocksize = 576 << (bs_code - 2);
  else if (bs_code == 6) blocksize = (int)br_u(b, 8) + 1;
  else if (bs_code == 7) blocksize = (int)br_u(b, 16) + 1;
  else blocksize = 256 << (bs_code - 8);
  if (sr_code == 12) br_u(b, 8); else if (sr_code == 13 || sr_code == 14) br_u(b, 16); else if (sr_code == 15) return FLAC_E_HEADER;
  int fbps = bps;
  switch (ss_code) { case 0: break; case 1: fbps = 8; break; case 2: fbps = 12; break; case 4: fbps = 16; break;
                     case 5: fbps = 20; break; case 6: fbps = 24; break; case 7: fbps = 32; break; default: return FLAC_E_HEADER; }
  int nch = ch_code < 8 ? ch_code + 1 : 2;
  if (ch_code > 10 || nch != ch || fbps != bps || blocksize > FLAC_MAX_BLOCK) return ch_code > 10 ? FLAC_E_HEADER : FLAC_E_UNSUP;
  size_t hdr_end = br_bytepos(b);
  if (hdr_end + 1 > size) return FLAC_E_TRUNC;
  if (flac_crc8(data + pos, hdr_end - pos) != data[hdr_end]) return FLAC_E_CRC;
  br_u(b, 8);
  h->blocksize = blocksize; h->ch_code = ch_code; h->nch = nch;
  return FLAC_OK;
}

/* Is `pos` a frame start as far as its header can tell?  The sync code, the reserved bits, codes consistent with the
 * stream (channels, sample size), a block size within STREAMINFO's maximum, a well-formed coded number, the CRC-8.
 * Returns the block size (1 .. max_block) or 0. */
FLAC_FN int flac_candidate(const uint8_t* data, size_t size, size_t pos, int ch, int bps, int max_block) {
  if (!flac_is_sync(data, size, pos)) return 0;
  BR b; flac_hdr h;
  if (flac_frame_header(&b, data, size, pos, ch, bps, &h) != FLAC_OK) return 0;
  return h.blocksize <= max_block ? h.blocksize : 0;
}

/* ---------------------------------------------------------------- chain (host side of the frame-parallel routes) */
/* Candidates sorted by start offset, each decoded on its own: start / end offsets, block size, decode status.  Walk the
 * stream from `first` the way wh_flac_decode's loop does: a frame is accepted when a candidate starts exactly where the
 * previous accepted frame ended and its own checks held (rc == 0, the CRC-16 among them).  The stream may end in at most
 * FLAC_TAIL bytes that do not start with a sync code (`tail` = the last min(size, FLAC_TAIL) bytes of the file); anything
 * else where no candidate starts breaks the chain.  (wh_flac_decode also lets a stream whose STREAMINFO total has been
 * reached end in a longer tail; the frame-parallel routes leave such a file to it.)  accepted[0 .. *n_acc) = the candidate
 * indices in stream order, *done = their samples per channel.  FLAC_OK or FLAC_E_REJECT. */
static inline int flac_chain(const int64_t* start, const int64_t* end, const int32_t* bs, const int32_t* rc, int n_cand,
                             size_t first, size_t size, const uint8_t* tail, uint64_t total, int32_t* accepted, int* n_acc,
                             int64_t* done) {
  const size_t tail_len = size < FLAC_TAIL ? size : FLAC_TAIL;
  size_t pos = first;
  int j = 0, n = 0;
  uint64_t got = 0;
  *n_acc = 0; *done = 0;
  while (pos + 2 <= size) {
    while (j < n_cand && (uint64_t)start[j] < (uint64_t)pos) ++j;
    if (j == n_cand || (uint64_t)start[j] != (uint64_t)pos) {
      const size_t rem = size - pos;
      if (rem > tail_len) return FLAC_E_REJECT;
      const uint8_t* t = tail + (tail_len - rem);
      if (t[0] == 0xFF && (t[1] & 0xFE) == 0xF8) return FLAC_E_REJECT;      /* a frame header that did not hold */
      break;
    }
    if (rc[j] != FLAC_OK || end[j] <= start[j] || (uint64_t)end[j] > (uint64_t)size) return FLAC_E_REJECT;
    accepted[n++] = j;
    got += (uint64_t)bs[j];
    pos = (size_t)end[j];
    ++j;
  }
  if (total && got < total) return FLAC_E_REJECT;
  *n_acc = n; *done = (int64_t)got;
  return FLAC_OK;
}

#endif /* WH_FLAC_CORE_H */

/* ================================================================ template part: FLAC_T, FLAC_SUFFIX */
#ifdef FLAC_T

#define FLAC_CAT2(a, b) a##b
#define FLAC_CAT(a, b) FLAC_CAT2(a, b)
#define FLAC_NAME(x) FLAC_CAT(x, FLAC_SUFFIX)
/* store a 64-bit value; a storage type that cannot hold it raises the flag (never with FLAC_T = int64_t) */
#define FLAC_PUT(lvalue, value, range) do { const int64_t v_ = (int64_t)(value); const FLAC_T t_ = (FLAC_T)v_; (lvalue) = t_; \
                                            if ((int64_t)t_ != v_) *(range) = 1; } while (0)
#define FLAC_S(i) s[(size_t)(i) * stride]

FLAC_FN int FLAC_NAME(flac_residual)(BR* b, FLAC_T* s, size_t stride, int blocksize, int order, int* range) {
  int method = (int)br_u(b, 2);
  if (method > 1) return FLAC_E_UNSUP;
  int pbits = method == 0 ? 4 : 5, esc = method == 0 ? 15 : 31;
  int porder = (int)br_u(b, 4);
  int nparts = 1 << porder;
  if ((blocksize >> porder) << porder != blocksize && porder > 0) return FLAC_E_HEADER;
  int i = order;
  for (int part = 0; part < nparts; ++part) {
    int count = (blocksize >> porder) - (part == 0 ? order : 0);
    if (count < 0 || i + count > blocksize) return FLAC_E_HEADER;
    int k = (int)br_u(b, pbits);
    if (k == esc) {
      int nb = (int)br_u(b, 5);
      for (int j = 0; j < count; ++j, ++i) FLAC_S(i) = (FLAC_T)(nb ? br_s(b, nb) : 0);
    } else {
      for (int j = 0; j < count; ++j, ++i) {
        uint32_t q = br_unary(b);
        uint64_t u = ((uint64_t)q << k) | br_u(b, k);
        FLAC_PUT(FLAC_S(i), (int64_t)(u >> 1) ^ -(int64_t)(u & 1), range);
      }
    }
    if (b->eof) return FLAC_E_TRUNC;
  }
  return FLAC_OK;
}

FLAC_FN int FLAC_NAME(flac_subframe)(BR* b, FLAC_T* s, size_t stride, int blocksize, int bps, int* range) {
  if (br_u(b, 1)) return FLAC_E_HEADER;
  int type = (int)br_u(b, 6);
  int wasted = 0;
  if (br_u(b, 1)) wasted = (int)br_unary(b) + 1;
  bps -= wasted;
  if (bps <= 0) return FLAC_E_HEADER;
  if (type == 0) {
    int64_t v = br_s64(b, bps);
    for (int i = 0; i < blocksize; ++i) FLAC_S(i) = (FLAC_T)v;
  } else if (type == 1) {
    for (int i = 0; i < blocksize; ++i) FLAC_S(i) = (FLAC_T)br_s64(b, bps);
  } else if (type >= 8 && type <= 12) {
    int order = type - 8;
    if (order > blocksize) return FLAC_E_HEADER;
    for (int i = 0; i < order; ++i) FLAC_S(i) = (FLAC_T)br_s64(b, bps);
    int rc = FLAC_NAME(flac_residual)(b, s, stride, blocksize, order, range);
    if (rc) return rc;
    /* wrapping arithmetic, as in the LPC branch below; h1 .. h4 = the four samples before i */
    uint64_t h1 = order >= 1 ? (uint64_t)(int64_t)FLAC_S(order - 1) : 0, h2 = order >= 2 ? (uint64_t)(int64_t)FLAC_S(order - 2) : 0,
             h3 = order >= 3 ? (uint64_t)(int64_t)FLAC_S(order - 3) : 0, h4 = order >= 4 ? (uint64_t)(int64_t)FLAC_S(order - 4) : 0;
    if (order > 0) for (int i = order; i < blocksize; ++i) {
      uint64_t v = (uint64_t)(int64_t)FLAC_S(i);
      switch (order) {
        case 1: v += h1; break;
        case 2: v += 2 * h1 - h2; break;
        case 3: v += 3 * h1 - 3 * h2 + h3; break;
        case 4: v += 4 * h1 - 6 * h2 + 4 * h3 - h4; break;
      }
      FLAC_PUT(FLAC_S(i), v, range);
      h4 = h3; h3 = h2; h2 = h1; h1 = (uint64_t)(int64_t)FLAC_S(i);
    }
  } else if (type >= 32) {
    int order = (type & 31) + 1;
    if (order > blocksize) return FLAC_E_HEADER;
    for (int i = 0; i < order; ++i) FLAC_S(i) = (FLAC_T)br_s64(b, bps);
    int prec = (int)br_u(b, 4) + 1;
    if (prec == 16) return FLAC_E_HEADER;
    int shift = br_s(b, 5);
    if (shift < 0) return FLAC_E_UNSUP;
    int32_t coef[32];
    for (int i = 0; i < order; ++i) coef[i] = br_s(b, prec);
    int rc = FLAC_NAME(flac_residual)(b, s, stride, blocksize, order, range);
    if (rc) return rc;
    for (int i = order; i < blocksize; ++i) {
      /* wrapping arithmetic: a valid stream never overflows 64 bits here, a corrupt one must not be undefined
         behaviour (its frame CRC / the MD5 reject it afterwards) */
      uint64_t sum = 0;
      for (int j = 0; j < order; ++j) sum += (uint64_t)(int64_t)coef[j] * (uint64_t)(int64_t)FLAC_S(i - 1 - j);
      FLAC_PUT(FLAC_S(i), (uint64_t)(int64_t)FLAC_S(i) + (uint64_t)((int64_t)sum >> shift), range);
    }
  } else {
    return FLAC_E_UNSUP;      /* reserved subframe types */
  }
  if (wasted) for (int i = 0; i < blocksize; ++i) FLAC_PUT(FLAC_S(i), (uint64_t)(int64_t)FLAC_S(i) << wasted, range);
  return b->eof ? FLAC_E_TRUNC : FLAC_OK;
}

/* One whole frame at `pos` (sync code seen by the caller): header, subframes, CRC-16, stereo decorrelation.  Sample i of
 * channel c goes to s[c * chan_off + i * stride].  *end = the offset behind the frame's CRC-16 once the body has been
 * parsed (also on FLAC_E_CRC), else `pos`.  A block size above bs_limit is refused before anything is stored. */
FLAC_FN int FLAC_NAME(flac_frame)(const uint8_t* data, size_t size, size_t pos, int ch, int bps, int bs_limit, FLAC_T* s,
                                  size_t chan_off, size_t stride, flac_hdr* h, size_t* end, int* range) {
  BR b;
  *end = pos;
  int rc = flac_frame_header(&b, data, size, pos, ch, bps, h);
  if (rc) return rc;
  if (h->blocksize > bs_limit) return FLAC_E_HEADER;
  const int blocksize = h->blocksize, ch_code = h->ch_code;
  for (int c = 0; c < h->nch; ++c) {
    int side = (ch_code == 8 && c == 1) || (ch_code == 9 && c == 0) || (ch_code == 10 && c == 1);
    rc = FLAC_NAME(flac_subframe)(&b, s + (size_t)c * chan_off, stride, blocksize, bps + side, range);
    if (rc) return rc;
  }
  br_align(&b);
  size_t body_end = br_bytepos(&b);
  if (body_end + 2 > size) return FLAC_E_TRUNC;
  *end = body_end + 2;
  if (flac_crc16(data + pos, body_end - pos) != (uint16_t)((data[body_end] << 8) | data[body_end + 1])) return FLAC_E_CRC;
  if (ch_code >= 8) {
    FLAC_T* w1 = s + chan_off;
    for (int i = 0; i < blocksize; ++i) {
      const uint64_t a = (uint64_t)(int64_t)FLAC_S(i), d = (uint64_t)(int64_t)w1[(size_t)i * stride];
      if (ch_code == 8) FLAC_PUT(w1[(size_t)i * stride], a - d, range);          /* left, side  -> right = left - side */
      else if (ch_code == 9) FLAC_PUT(FLAC_S(i), a + d, range);                  /* side, right -> left = right + side */
      else {                                                                     /* mid, side */
        const uint64_t mid = (a << 1) | (d & 1);
        FLAC_PUT(FLAC_S(i), (int64_t)(mid + d) >> 1, range);
        FLAC_PUT(w1[(size_t)i * stride], (int64_t)(mid - d) >> 1, range);
      }
    }
  }
  return FLAC_OK;
}

#undef FLAC_S
#undef FLAC_PUT
#undef FLAC_NAME
#undef FLAC_CAT
#undef FLAC_CAT2
#undef FLAC_T
#undef FLAC_SUFFIX
#endif /* FLAC_T */
