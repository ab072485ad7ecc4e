/* Host side of the input pipeline (include/satt_io.h): CRC-32C, TFRecord framing, tf.train.Example indexing, target
 * preparation.  Plain C for the CPU cores that feed the GPU: the 8.3 ms train step consumes ~3 850 utterances/s, a
 * byte-at-a-time Python checksum delivered 11. */
#include "../../include/satt_io.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <errno.h>
#include <string.h>

#if defined(__x86_64__)
#include <nmmintrin.h>
#define SATT_X86 1
#endif

int satt_io_version(void) { return 2; }
/* errno of the last SATT_IO_E_IO this thread returned (fopen / fread failure) */
static __thread int io_errno_;
int satt_io_last_errno(void) { return io_errno_; }

/* ------------------------------------------------------------------------------------------------ CRC-32C */
static uint32_t T8[8][256];
static volatile int t8_ready = 0;

static void t8_init(void) {
  if (t8_ready) return;
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
    T8[0][i] = c;
  }
  for (uint32_t i = 0; i < 256; ++i)
    for (int s = 1; s < 8; ++s) T8[s][i] = (T8[s - 1][i] >> 8) ^ T8[0][T8[s - 1][i] & 0xFFu];
  __sync_synchronize();
  t8_ready = 1; /* idempotent: two threads racing here write identical tables */
}

static uint32_t crc_sw(uint32_t c, const uint8_t* p, size_t n) {
  t8_init();
  while (n && ((uintptr_t)p & 7u)) { c = T8[0][(c ^ *p++) & 0xFFu] ^ (c >> 8); --n; }
  while (n >= 8) { /* slicing-by-8 */
    uint64_t w;
    memcpy(&w, p, 8);
    w ^= c;
    c = T8[7][w & 0xFF] ^ T8[6][(w >> 8) & 0xFF] ^ T8[5][(w >> 16) & 0xFF] ^ T8[4][(w >> 24) & 0xFF] ^
        T8[3][(w >> 32) & 0xFF] ^ T8[2][(w >> 40) & 0xFF] ^ T8[1][(w >> 48) & 0xFF] ^ T8[0][(w >> 56) & 0xFF];
    p += 8; n -= 8;
  }
  while (n--) c = T8[0][(c ^ *p++) & 0xFFu] ^ (c >> 8);
  return c;
}

#ifdef SATT_X86
/* one crc32 chain: 8 bytes per 3-cycle instruction, ~8 GB/s - a 256 KB mel record in ~30 us, far below its file read */
__attribute__((target("sse4.2"))) static uint32_t crc_hw_run(uint32_t c, const uint8_t* p, size_t n) {
  uint64_t c64 = c;
  while (n && ((uintptr_t)p & 7u)) { c64 = _mm_crc32_u8((uint32_t)c64, *p++); --n; }
  while (n >= 8) { uint64_t w; memcpy(&w, p, 8); c64 = _mm_crc32_u64(c64, w); p += 8; n -= 8; }
  while (n--) c64 = _mm_crc32_u8((uint32_t)c64, *p++);
  return (uint32_t)c64;
}
static int hw_ok(void) {
  static int v = -1;
  if (v < 0) v = __builtin_cpu_supports("sse4.2") ? 1 : 0;
  return v;
}
#else
static int hw_ok(void) { return 0; }
#endif

int satt_io_crc32c_hw(void) { return hw_ok(); }

uint32_t satt_crc32c_extend(uint32_t crc, const void* data, size_t n) {
  uint32_t c = ~crc;
#ifdef SATT_X86
  if (hw_ok()) return ~crc_hw_run(c, (const uint8_t*)data, n);
#endif
  return ~crc_sw(c, (const uint8_t*)data, n);
}
uint32_t satt_crc32c(const void* data, size_t n) { return satt_crc32c_extend(0u, data, n); }
uint32_t satt_masked_crc32c(const void* data, size_t n) {
  const uint32_t c = satt_crc32c(data, n);
  return ((c >> 15) | (c << 17)) + 0xA282EAD8u;
}
/* (test hook: the table path regardless of the CPU) */
uint32_t satt_crc32c_sw(const void* data, size_t n) { return ~crc_sw(~0u, (const uint8_t*)data, n); }

/* ------------------------------------------------------------------------------------------------ TFRecord framing */
static uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }

int64_t satt_tfrecord_index(const uint8_t* buf, size_t n, int verify, int64_t* offsets, int64_t* lengths, int64_t max_records) {
  if ((!buf && n) || !offsets || !lengths) return SATT_IO_E_BADARG;
  size_t pos = 0;
  int64_t k = 0;
  while (pos < n) {
    if (n - pos < 12) return SATT_IO_E_TRUNCATED_HEADER;
    const uint64_t len = rd64(buf + pos);
    if (verify && satt_masked_crc32c(buf + pos, 8) != rd32(buf + pos + 8)) return SATT_IO_E_CORRUPT_LENGTH;
    pos += 12;
    if (len > n - pos || n - pos - len < 4) return SATT_IO_E_TRUNCATED_RECORD;
    if (verify && satt_masked_crc32c(buf + pos, (size_t)len) != rd32(buf + pos + len)) return SATT_IO_E_CORRUPT_PAYLOAD;
    if (k >= max_records) return SATT_IO_E_TOO_MANY;
    offsets[k] = (int64_t)pos; lengths[k] = (int64_t)len; ++k;
    pos += (size_t)len + 4;
  }
  return k;
}

int64_t satt_tfrecord_load(const char* path, int verify, uint8_t* buf, size_t cap, int64_t* nbytes, int64_t* offsets,
                           int64_t* lengths, int64_t max_records) {
  if (!path || !buf || !nbytes) return SATT_IO_E_BADARG;
  FILE* f = fopen(path, "rb");
  if (!f) { io_errno_ = errno; return SATT_IO_E_IO; }
  size_t got = fread(buf, 1, cap, f);
  if (got < cap && ferror(f)) { io_errno_ = errno; fclose(f); return SATT_IO_E_IO; }
  int64_t total = (int64_t)got;
  if (got == cap) {                       /* possibly more: report the real size so the caller can retry */
    if (fgetc(f) != EOF) {
      fseek(f, 0, SEEK_END);
      *nbytes = (int64_t)ftell(f);
      fclose(f);
      return SATT_IO_E_TOO_MANY;
    }
  }
  fclose(f);
  *nbytes = total;
  return satt_tfrecord_index(buf, got, verify, offsets, lengths, max_records);
}

/* ------------------------------------------------------------------------------------------------ protobuf wire format */
typedef struct { const uint8_t* p; const uint8_t* end; } cur_t;

static int varint(cur_t* c, uint64_t* out) {
  uint64_t x = 0;
  for (int shift = 0; shift < 70; shift += 7) {
    if (c->p >= c->end) return 0;
    const uint8_t b = *c->p++;
    x |= (uint64_t)(b & 0x7F) << (shift < 64 ? shift : 63);
    if (!(b & 0x80)) { *out = x; return 1; }
  }
  return 0;
}
/* next field of a message: number, wire type, and for type 2 the body [*body, *body + *blen); for 0 / 1 / 5 the value */
static int field(cur_t* c, uint32_t* num, uint32_t* wt, uint64_t* val, const uint8_t** body, uint64_t* blen) {
  uint64_t key;
  if (!varint(c, &key)) return 0;
  *num = (uint32_t)(key >> 3); *wt = (uint32_t)(key & 7);
  switch (*wt) {
    case 0: return varint(c, val);
    case 1: if (c->end - c->p < 8) return 0; *val = rd64(c->p); c->p += 8; return 1;
    case 5: if (c->end - c->p < 4) return 0; *val = rd32(c->p); c->p += 4; return 1;
    case 2:
      if (!varint(c, blen) || *blen > (uint64_t)(c->end - c->p)) return 0;
      *body = c->p; c->p += *blen; return 1;
    default: return 0;
  }
}

static int list_summary(const uint8_t* base, const uint8_t* body, uint64_t blen, int kind, satt_example_feature* f) {
  cur_t c = {body, body + blen};
  uint32_t num, wt; uint64_t val = 0, l2 = 0; const uint8_t* b2 = 0;
  int64_t count = 0, runs = 0, unpacked = 0;
  f->val_off = (int64_t)(body - base); f->val_len = (int64_t)blen; f->packed = 0; f->first_int = 0;
  while (c.p < c.end) {
    if (!field(&c, &num, &wt, &val, &b2, &l2)) return 0;
    if (num != 1) continue;
    if (kind == 1) {
      if (wt != 2) return 0;
      if (count == 0) { f->val_off = (int64_t)(b2 - base); f->val_len = (int64_t)l2; }
      ++count;
    } else if (wt == 2) {             /* packed run */
      ++runs;
      if (kind == 2) { if (l2 % 4) return 0; count += (int64_t)(l2 / 4); }
      else { cur_t q = {b2, b2 + l2}; uint64_t v; while (q.p < q.end) { if (!varint(&q, &v)) return 0; if (!count) f->first_int = (int64_t)v; ++count; } }
      if (runs == 1) { f->val_off = (int64_t)(b2 - base); f->val_len = (int64_t)l2; }
    } else { if (kind == 3 && wt == 0 && !count) f->first_int = (int64_t)val; ++unpacked; ++count; }
  }
  if (kind != 1) {
    f->packed = (runs == 1 && unpacked == 0) ? 1 : 0;
    if (!f->packed) { f->val_off = (int64_t)(body - base); f->val_len = (int64_t)blen; }   /* mixed / unpacked: the list body */
  }
  f->count = count;
  return 1;
}

int64_t satt_example_index(const uint8_t* payload, size_t n, satt_example_feature* feats, int64_t max_features) {
  if (!payload || !feats) return SATT_IO_E_BADARG;
  cur_t ex = {payload, payload + n};
  uint32_t num, wt; uint64_t val = 0, blen = 0; const uint8_t* body = 0;
  int64_t k = 0;
  while (ex.p < ex.end) {
    if (!field(&ex, &num, &wt, &val, &body, &blen)) return SATT_IO_E_MALFORMED;
    if (num != 1 || wt != 2) continue;                       /* Example.features */
    cur_t fs = {body, body + blen};
    while (fs.p < fs.end) {
      uint64_t elen = 0; const uint8_t* ebody = 0;
      if (!field(&fs, &num, &wt, &val, &ebody, &elen)) return SATT_IO_E_MALFORMED;
      if (num != 1 || wt != 2) continue;                     /* one map entry: key = 1, value = 2 */
      cur_t en = {ebody, ebody + elen};
      const uint8_t *name = 0, *feat = 0; uint64_t nlen = 0, flen = 0; int have_feat = 0;
      while (en.p < en.end) {
        uint64_t l3 = 0; const uint8_t* b3 = 0;
        if (!field(&en, &num, &wt, &val, &b3, &l3)) return SATT_IO_E_MALFORMED;
        if (wt != 2) continue;
        if (num == 1) { name = b3; nlen = l3; }
        else if (num == 2) { feat = b3; flen = l3; have_feat = 1; }
      }
      if (!name || !have_feat) continue;
      if (k >= max_features) return SATT_IO_E_TOO_MANY;
      satt_example_feature* f = &feats[k];
      memset(f, 0, sizeof(*f));
      f->name_off = (int64_t)(name - payload); f->name_len = (int64_t)nlen;
      cur_t fc = {feat, feat + flen};
      while (fc.p < fc.end) {                                /* the oneof: the LAST list present wins (proto semantics) */
        uint64_t l4 = 0; const uint8_t* b4 = 0;
        if (!field(&fc, &num, &wt, &val, &b4, &l4)) return SATT_IO_E_MALFORMED;
        if (wt != 2 || num < 1 || num > 3) continue;
        f->kind = (int32_t)num;
        if (!list_summary(payload, b4, l4, (int)num, f)) return SATT_IO_E_MALFORMED;
      }
      ++k;
    }
  }
  return k;
}

int64_t satt_example_int64s(const uint8_t* body, size_t n, int packed, int64_t* out, int64_t max_out) {
  if ((!body && n) || !out) return SATT_IO_E_BADARG;
  cur_t c = {body, body + n};
  int64_t k = 0;
  uint64_t v;
  if (packed) {
    while (c.p < c.end) {
      if (!varint(&c, &v)) return SATT_IO_E_MALFORMED;
      if (k >= max_out) return SATT_IO_E_TOO_MANY;
      out[k++] = (int64_t)v;
    }
    return k;
  }
  uint32_t num, wt; uint64_t l2 = 0; const uint8_t* b2 = 0;
  while (c.p < c.end) {
    if (!field(&c, &num, &wt, &v, &b2, &l2)) return SATT_IO_E_MALFORMED;
    if (num != 1) continue;
    if (wt == 0) { if (k >= max_out) return SATT_IO_E_TOO_MANY; out[k++] = (int64_t)v; }
    else if (wt == 2) {
      cur_t q = {b2, b2 + l2};
      while (q.p < q.end) {
        if (!varint(&q, &v)) return SATT_IO_E_MALFORMED;
        if (k >= max_out) return SATT_IO_E_TOO_MANY;
        out[k++] = (int64_t)v;
      }
    }
  }
  return k;
}

int64_t satt_example_bytes(const uint8_t* body, size_t n, int64_t* offsets, int64_t* lengths, int64_t max_out) {
  if ((!body && n) || !offsets || !lengths) return SATT_IO_E_BADARG;
  cur_t c = {body, body + n};
  uint32_t num, wt; uint64_t v = 0, l2 = 0; const uint8_t* b2 = 0;
  int64_t k = 0;
  while (c.p < c.end) {
    if (!field(&c, &num, &wt, &v, &b2, &l2)) return SATT_IO_E_MALFORMED;
    if (num != 1 || wt != 2) continue;
    if (k >= max_out) return SATT_IO_E_TOO_MANY;
    offsets[k] = (int64_t)(b2 - body); lengths[k] = (int64_t)l2; ++k;
  }
  return k;
}

/* ------------------------------------------------------------------------------------------------ one utterance */
static int64_t read_whole(const char* path, uint8_t* buf, size_t cap, int64_t* size) {
  FILE* f = fopen(path, "rb");
  if (!f) { io_errno_ = errno; return SATT_IO_E_IO; }
  size_t got = fread(buf, 1, cap, f);
  if (got < cap && ferror(f)) { io_errno_ = errno; fclose(f); return SATT_IO_E_IO; }
  if (got == cap && fgetc(f) != EOF) {
    fseek(f, 0, SEEK_END);
    *size = (int64_t)ftell(f);
    fclose(f);
    return SATT_IO_E_TOO_MANY;
  }
  fclose(f);
  *size = (int64_t)got;
  return 0;
}
static const satt_example_feature* find(const uint8_t* payload, const satt_example_feature* fs, int64_t n, const char* name) {
  const size_t ln = strlen(name);
  for (int64_t i = 0; i < n; ++i)
    if ((size_t)fs[i].name_len == ln && !memcmp(payload + fs[i].name_off, name, ln)) return &fs[i];
  return 0;
}
static int64_t int_of(const uint8_t* payload, const satt_example_feature* fs, int64_t n, const char* name, int64_t dflt, int* ok) {
  const satt_example_feature* f = find(payload, fs, n, name);
  if (!f || f->kind != 3 || f->count < 1) { if (ok) *ok = 0; return dflt; }
  return f->first_int;
}

int64_t satt_utterance_load(const char* source_path, const char* target_path, int verify, int64_t r, uint8_t* arena, size_t cap,
                            satt_utterance* out) {
  if (!source_path || !target_path || !arena || !out || r < 1) return SATT_IO_E_BADARG;
  memset(out, 0, sizeof(*out));
  int64_t e = read_whole(source_path, arena, cap, &out->src_bytes);
  if (e == SATT_IO_E_IO) return e;
  const int src_over = (e == SATT_IO_E_TOO_MANY);
  const size_t used = src_over ? cap : (size_t)out->src_bytes;
  e = read_whole(target_path, arena + used, cap - used, &out->tgt_bytes);
  if (e == SATT_IO_E_IO) return e;
  if (src_over || e == SATT_IO_E_TOO_MANY) {
    if (src_over) {                        /* the target's size is still unknown: measure it */
      FILE* f = fopen(target_path, "rb");
      if (!f) { io_errno_ = errno; return SATT_IO_E_IO; }
      fseek(f, 0, SEEK_END); out->tgt_bytes = (int64_t)ftell(f); fclose(f);
    }
    return SATT_IO_E_TOO_MANY;
  }
  enum { MAXF = 32 };
  int64_t offs[2], lens[2];
  satt_example_feature fs[MAXF];
  /* ---- source record */
  {
    int64_t o[8], l[8];
    int64_t k = satt_tfrecord_index(arena, (size_t)out->src_bytes, verify, o, l, 8);
    if (k == SATT_IO_E_TOO_MANY) k = 9;      /* more than 8 records: a multi-record file - the caller takes the general path */
    if (k < 0) return k;
    out->src_records = k;
    if (k < 1) return SATT_IO_E_BADARG;
    offs[0] = o[0]; lens[0] = l[0];
  }
  {
    int64_t o[8], l[8];
    int64_t k = satt_tfrecord_index(arena + out->src_bytes, (size_t)out->tgt_bytes, verify, o, l, 8);
    if (k == SATT_IO_E_TOO_MANY) k = 9;
    if (k < 0) return k;
    out->tgt_records = k;
    if (k < 1) return SATT_IO_E_BADARG;
    offs[1] = out->src_bytes + o[0]; lens[1] = l[0];
  }
  const uint8_t* ps = arena + offs[0];
  int64_t n = satt_example_index(ps, (size_t)lens[0], fs, MAXF);
  if (n < 0) return n;
  int ok = 1;
  out->id = int_of(ps, fs, n, "id", 0, &ok);
  out->source_length = int_of(ps, fs, n, "source_length", 0, &ok);
  out->speaker_id = int_of(ps, fs, n, "speaker_id", -1, 0);
  out->age = int_of(ps, fs, n, "age", -1, 0);
  out->gender = int_of(ps, fs, n, "gender", -1, 0);
  const satt_example_feature* f = find(ps, fs, n, "key");
  if (!f || f->kind != 1 || f->count < 1) return SATT_IO_E_BADARG;
  out->key_off = offs[0] + f->val_off; out->key_len = f->val_len;
  f = find(ps, fs, n, "text");
  if (f && f->kind == 1 && f->count >= 1) { out->text_off = offs[0] + f->val_off; out->text_len = f->val_len; }
  f = find(ps, fs, n, "source");
  if (!ok || !f || f->kind != 1 || f->count < 1 || f->val_len % 8) return SATT_IO_E_BADARG;
  out->source_off = offs[0] + f->val_off; out->source_count = f->val_len / 8;
  /* a length beyond the ids the record holds would reach the device kernels as an out-of-range sequence length */
  if (out->source_length < 0 || out->source_length > out->source_count) return SATT_IO_E_BADARG;
  out->accent_off = 0; out->accent_count = -1;
  f = find(ps, fs, n, "accent_type");
  if (f && f->count >= 1) {        /* one accentual-type id per symbol: exactly source_length int64 values */
    if (f->kind != 1 || f->val_len % 8 || f->val_len / 8 != out->source_length) return SATT_IO_E_ACCENT;
    out->accent_off = offs[0] + f->val_off; out->accent_count = f->val_len / 8;
  }
  /* ---- target record */
  const uint8_t* pt = arena + offs[1];
  n = satt_example_index(pt, (size_t)lens[1], fs, MAXF);
  if (n < 0) return n;
  ok = 1;
  out->target_id = int_of(pt, fs, n, "id", 0, &ok);
  out->target_length = int_of(pt, fs, n, "target_length", 0, &ok);
  out->mel_width = int_of(pt, fs, n, "mel_width", 0, &ok);
  f = find(pt, fs, n, "mel");
  if (!ok || !f || f->kind != 1 || f->count < 1 || f->val_len % 4) return SATT_IO_E_BADARG;
  out->mel_off = offs[1] + f->val_off; out->mel_count = f->val_len / 4;
  /* bounds BEFORE the product (a crafted record must not overflow a signed 64-bit multiplication): a width of at most 4096
   * channels, and no more frames than the value has floats */
  if (out->target_length < 0 || out->mel_width < 1 || out->mel_width > 4096 || out->target_length > out->mel_count ||
      out->mel_count != out->target_length * out->mel_width) return SATT_IO_E_BADARG;
  out->prepared_length = satt_prepared_length(out->target_length, r);
  return 0;
}

/* ------------------------------------------------------------------------------------------------ native reader */
enum { SL_FREE = 0, SL_QUEUED, SL_RUNNING, SL_DONE, SL_LEASED };
typedef struct {
  int state;
  int64_t ticket, status;
  char *src, *tgt;
  uint8_t* arena;
  size_t cap;
  satt_utterance u;
} slot_t;
struct satt_reader {
  pthread_mutex_t mu;
  pthread_cond_t work, done;
  pthread_t* th;
  slot_t* sl;
  int workers, slots, verify, stop;
  int64_t r;
  int64_t submitted, started, delivered;   /* tickets: [delivered, submitted) outstanding, [started, submitted) not yet picked up */
};

static void* reader_main(void* arg) {
  satt_reader* rd = (satt_reader*)arg;
  pthread_mutex_lock(&rd->mu);
  for (;;) {
    while (!rd->stop && rd->started >= rd->submitted) pthread_cond_wait(&rd->work, &rd->mu);
    if (rd->stop) break;
    slot_t* s = &rd->sl[rd->started++ % rd->slots];
    s->state = SL_RUNNING;
    pthread_mutex_unlock(&rd->mu);
    int64_t e = satt_utterance_load(s->src, s->tgt, rd->verify, rd->r, s->arena, s->cap, &s->u);
    if (e == SATT_IO_E_TOO_MANY) {           /* grow this slot's buffer to the files' sizes and read again */
      const size_t need = (size_t)(s->u.src_bytes + s->u.tgt_bytes) + 4096;
      uint8_t* nb = (uint8_t*)realloc(s->arena, need);
      if (nb) { s->arena = nb; s->cap = need; e = satt_utterance_load(s->src, s->tgt, rd->verify, rd->r, s->arena, s->cap, &s->u); }
    }
    pthread_mutex_lock(&rd->mu);
    s->status = e;
    s->state = SL_DONE;
    pthread_cond_broadcast(&rd->done);
  }
  pthread_mutex_unlock(&rd->mu);
  return 0;
}

satt_reader* satt_reader_create(int workers, int slots, size_t arena_bytes, int verify, int64_t r) {
  if (workers < 1 || slots < 1 || r < 1) return 0;
  satt_reader* rd = (satt_reader*)calloc(1, sizeof(*rd));
  if (!rd) return 0;
  rd->workers = workers; rd->slots = slots; rd->verify = verify; rd->r = r;
  rd->sl = (slot_t*)calloc((size_t)slots, sizeof(slot_t));
  rd->th = (pthread_t*)calloc((size_t)workers, sizeof(pthread_t));
  if (!rd->sl || !rd->th) { free(rd->sl); free(rd->th); free(rd); return 0; }
  if (arena_bytes < 4096) arena_bytes = 4096;
  for (int i = 0; i < slots; ++i) { rd->sl[i].arena = (uint8_t*)malloc(arena_bytes); rd->sl[i].cap = rd->sl[i].arena ? arena_bytes : 0; }
  pthread_mutex_init(&rd->mu, 0);
  pthread_cond_init(&rd->work, 0);
  pthread_cond_init(&rd->done, 0);
  int started = 0;
  for (; started < workers; ++started)
    if (pthread_create(&rd->th[started], 0, reader_main, rd)) break;
  if (started < 1) { rd->workers = 0; satt_reader_destroy(rd); return 0; }
  rd->workers = started;
  return rd;
}

int64_t satt_reader_submit(satt_reader* rd, const char* source_path, const char* target_path) {
  if (!rd || !source_path || !target_path) return SATT_IO_E_BADARG;
  pthread_mutex_lock(&rd->mu);
  slot_t* s = &rd->sl[rd->submitted % rd->slots];
  if (s->state != SL_FREE || !s->arena) { pthread_mutex_unlock(&rd->mu); return s->arena ? SATT_IO_E_TOO_MANY : SATT_IO_E_BADARG; }
  free(s->src); free(s->tgt);
  s->src = strdup(source_path); s->tgt = strdup(target_path);
  if (!s->src || !s->tgt) { pthread_mutex_unlock(&rd->mu); return SATT_IO_E_BADARG; }
  s->ticket = rd->submitted++;
  s->state = SL_QUEUED;
  const int64_t t = s->ticket;
  pthread_cond_signal(&rd->work);
  pthread_mutex_unlock(&rd->mu);
  return t;
}

int64_t satt_reader_next(satt_reader* rd, satt_utterance* out, uint8_t** arena, int64_t* status) {
  if (!rd || !out || !arena || !status) return SATT_IO_E_BADARG;
  pthread_mutex_lock(&rd->mu);
  if (rd->delivered >= rd->submitted) { pthread_mutex_unlock(&rd->mu); return SATT_IO_E_BADARG; }
  slot_t* s = &rd->sl[rd->delivered % rd->slots];
  while (s->state != SL_DONE) pthread_cond_wait(&rd->done, &rd->mu);
  s->state = SL_LEASED;
  rd->delivered++;
  *out = s->u; *arena = s->arena; *status = s->status;
  const int64_t t = s->ticket;
  pthread_mutex_unlock(&rd->mu);
  return t;
}

int satt_reader_release(satt_reader* rd, int64_t ticket) {
  if (!rd || ticket < 0) return SATT_IO_E_BADARG;
  pthread_mutex_lock(&rd->mu);
  slot_t* s = &rd->sl[ticket % rd->slots];
  const int ok = (s->state == SL_LEASED && s->ticket == ticket);
  if (ok) s->state = SL_FREE;
  pthread_mutex_unlock(&rd->mu);
  return ok ? 0 : SATT_IO_E_BADARG;
}

int64_t satt_reader_outstanding(const satt_reader* rd) { return rd ? rd->submitted - rd->delivered : 0; }

void satt_reader_destroy(satt_reader* rd) {
  if (!rd) return;
  pthread_mutex_lock(&rd->mu);
  rd->stop = 1;
  pthread_cond_broadcast(&rd->work);
  pthread_mutex_unlock(&rd->mu);
  for (int i = 0; i < rd->workers; ++i) pthread_join(rd->th[i], 0);
  for (int i = 0; i < rd->slots; ++i) { free(rd->sl[i].arena); free(rd->sl[i].src); free(rd->sl[i].tgt); }
  pthread_mutex_destroy(&rd->mu); pthread_cond_destroy(&rd->work); pthread_cond_destroy(&rd->done);
  free(rd->sl); free(rd->th); free(rd);
}

/* ------------------------------------------------------------------------------------------------ target preparation */
typedef float __attribute__((aligned(1))) uf32;   /* the mel bytes sit wherever the record put them */

int64_t satt_prepared_length(int64_t T, int64_t r) {
  if (T < 0 || r < 1) return SATT_IO_E_BADARG;
  int64_t L = T + 2 * r;
  if (L % r) L = (L / r + 1) * r;
  return L;
}

int64_t satt_prepare_mel(const float* mel_, int64_t T, int64_t width, const float* avg, int64_t navg, const float* std_,
                         int64_t nstd, int64_t r, float silence, float* out, int64_t rows_out) {
  const uf32* mel = (const uf32*)mel_;
  if (!out || (!mel && T) || !avg || !std_ || width < 1 || (navg != 1 && navg != width) || (nstd != 1 && nstd != width))
    return SATT_IO_E_BADARG;
  const int64_t L = satt_prepared_length(T, r);
  if (L < 0 || rows_out < L) return SATT_IO_E_BADARG;
  for (int64_t j = 0; j < nstd; ++j)
    if (!(std_[j] > 0.f)) return SATT_IO_E_BADARG;
  for (int64_t i = 0; i < r * width; ++i) out[i] = silence;
  float* o = out + r * width;
  /* (mel - avg) / std with a true division: bit-identical to the numpy expression of the Python path */
  if (navg == 1 && nstd == 1) {
    const float a = avg[0], s = std_[0];
    for (int64_t i = 0; i < T * width; ++i) o[i] = (mel[i] - a) / s;
  } else {
    for (int64_t t = 0; t < T; ++t) {
      const uf32* m = mel + t * width;
      float* q = o + t * width;
      for (int64_t j = 0; j < width; ++j) q[j] = (m[j] - avg[navg == 1 ? 0 : j]) / std_[nstd == 1 ? 0 : j];
    }
  }
  float* tail = out + (r + T) * width;
  const int64_t ntail = (rows_out - r - T) * width;
  for (int64_t i = 0; i < ntail; ++i) tail[i] = silence;
  return L;
}
