// tokenize.hip -- the device half of tokenising a corpus for DataLoader.tfidf (graphconvgeo_amd/
// tfidf.py, tokenize_corpus_device): sklearn's analyzer at ngram_range (1, 1) for the patterns
// (?u)\b\w\w+\b and (?u)(?<![#@])\b\w\w+\b over the corpus as UTF-8 bytes. findall on either is a
// run rule: a token is a maximal run of word characters of at least two code points, and with the
// lookbehind a run whose preceding code point is '#' or '@' is dropped whole. The documents arrive
// joined by one NUL each; NUL is no word character and neither '#' nor '@', so the joined buffer
// tokenises as one text and the documents only decide the per-document counts.
//
// mark: per byte, decode the code point at lead bytes, look its class up in the bitmap the host
// built from the regex engine, flag token starts, run ends and NULs; per-tile counts. spans: the
// tokens' start offsets and the documents' token offsets. hash / sort / verify / number: the term
// dictionary (ids in order of first appearance), exact whatever the hash does because every token
// is compared byte by byte with its run's representative. remap: the host's per-term action
// (drop, -1, column) and the final doc_ptr. Integers only; no atomics that carry a value.
//
// The same stages parse the @mentions of the mention graph (graphconvgeo_amd/mentions.py,
// mention_incidences_device): the marking's other rule flags the names the regex of data.py:311
// finds, a rule over three ASCII byte classes, and the dictionary folds A-Z where it hashes and
// compares, so that the spellings of one name are one term.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "scratch.h"

using namespace gcg;

namespace {

constexpr int kTile = GCG_TOKENIZE_TILE_BYTES;  // bytes of text per workgroup
constexpr int kThreads = 256;
constexpr int kPerThread = kTile / kThreads;  // 16: one dwordx4 per lane, 1 KiB per wave load
constexpr int kBack = 16, kFwd = 16;          // LDS halo; 4 bytes back and 7 forward are read
constexpr uint32_t kCodePoints = 0x110000;

enum : uint8_t { kStart = 1, kRunEnd = 2, kNul = 4 };

typedef unsigned long long u64;

__device__ __forceinline__ bool is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }

// The code point whose lead byte is s[0] and its byte length, from the lead byte alone: whatever
// the bytes are, at most s[3] is read.
__device__ __forceinline__ uint32_t decode(const uint8_t* s, int* len) {
  const uint32_t b0 = s[0];
  if (b0 < 0x80u) { *len = 1; return b0; }
  if (b0 < 0xE0u) { *len = 2; return ((b0 & 0x1Fu) << 6) | (s[1] & 0x3Fu); }
  if (b0 < 0xF0u) { *len = 3; return ((b0 & 0x0Fu) << 12) | ((s[1] & 0x3Fu) << 6) | (s[2] & 0x3Fu); }
  *len = 4;
  return ((b0 & 0x07u) << 18) | ((s[1] & 0x3Fu) << 12) | ((s[2] & 0x3Fu) << 6) | (s[3] & 0x3Fu);
}

// \w of the host's regex engine: ASCII from the table's first four words (in LDS), the rest from
// the table in global memory (136 KiB, read-only: it lives in L2).
__device__ __forceinline__ bool is_word(uint32_t cp, const uint32_t* ascii,
                                        const uint32_t* __restrict__ table) {
  if (cp < 128u) return (ascii[cp >> 5] >> (cp & 31u)) & 1u;
  if (cp >= kCodePoints) return false;
  return (table[cp >> 5] >> (cp & 31u)) & 1u;
}

// The byte classes of the mention regex (?<=^|(?<=[^a-zA-Z0-9-_\.]))@([A-Za-z]+[A-Za-z0-9_]+):
// L = [A-Za-z], N = L, digits and '_' (a name's bytes), P = N, '-' and '.' (what may not precede
// the '@'). All ASCII: no byte of a multi-byte code point is in any of them.
__device__ __forceinline__ bool is_letter(uint32_t b) { return ((b | 0x20u) - 'a') < 26u; }
__device__ __forceinline__ bool is_name(uint32_t b) {
  return is_letter(b) || (b - '0') < 10u || b == '_';
}
__device__ __forceinline__ bool is_before_name(uint32_t b) {
  return is_name(b) || b == '-' || b == '.';
}

// The flag of byte s[0] under the mention rule; s[-2] .. s[1] are read. '@' opens a mention
// where the byte before it is not in P (a document's first '@' follows a NUL, or the start of
// the text, which reads as NUL) and a letter and a name byte follow; the name is the run of N
// from the letter on, so it starts here where s[-1] is such an '@' and ends at the first byte
// outside N. Runs of N that are no name end with kRunEnd too: only what follows a kStart is read.
__device__ __forceinline__ uint8_t mention_flag(const uint8_t* s) {
  const uint32_t b = s[0];
  uint8_t f = 0;
  if (is_name(b)) {
    if (is_letter(b) && s[-1] == '@' && !is_before_name(s[-2]) && is_name(s[1])) f = kStart;
  } else if (is_name(s[-1])) {
    f = kRunEnd;
  }
  return b == 0 ? f | kNul : f;
}

// One tile per workgroup. The tile and its halo go to LDS with one 16-byte load per lane; bytes
// outside [0, n) read as NUL, so the text starts and ends as a document does. Byte p of the tile
// is lane p % 256's, so a wave reads 64 consecutive LDS bytes. flags[g] for every g below
// round16(n); cnt[tile] = token starts | NULs << 32. kMentions: the mention rule instead of the
// word runs (no table, no lookbehind).
template <bool kMentions>
__global__ __launch_bounds__(kThreads) void tokenize_mark_kernel(
    int64_t n, const uint8_t* __restrict__ text, const uint32_t* __restrict__ table, int lookbehind,
    uint8_t* __restrict__ flags, u64* __restrict__ cnt, int64_t n_tiles) {
  __shared__ __align__(16) uint8_t lds[kBack + kTile + kFwd];
  __shared__ uint32_t ascii[4];
  __shared__ unsigned int n_start, n_nul;
  uint8_t* s = lds + kBack;
  const int64_t n16 = (n + 15) & ~int64_t{15};
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * kTile;
    {
      const int64_t g = t0 + static_cast<int64_t>(threadIdx.x) * kPerThread;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (g < n16) v = *reinterpret_cast<const uint4*>(text + g);
      *reinterpret_cast<uint4*>(s + threadIdx.x * kPerThread) = v;
    }
    if (threadIdx.x < kBack + kFwd) {
      const int off = threadIdx.x < kBack ? static_cast<int>(threadIdx.x) - kBack
                                          : kTile + static_cast<int>(threadIdx.x) - kBack;
      const int64_t g = t0 + off;
      s[off] = (g >= 0 && g < n) ? text[g] : uint8_t{0};
    }
    if (!kMentions && threadIdx.x < 4) ascii[threadIdx.x] = table[threadIdx.x];
    if (threadIdx.x == 0) { n_start = 0; n_nul = 0; }
    __syncthreads();
    if (t0 + kTile > n) {  // the last tile: what the 16-byte loads brought in past n is NUL
      for (int p = threadIdx.x; p < kTile; p += kThreads)
        if (t0 + p >= n) s[p] = 0;
      __syncthreads();
    }
    unsigned int my_start = 0, my_nul = 0;
#pragma unroll 4
    for (int k = 0; k < kPerThread; ++k) {
      const int p = k * kThreads + threadIdx.x;
      const int64_t g = t0 + p;
      if (g >= n16) break;
      uint8_t f = 0;
      const uint32_t b = s[p];
      if (kMentions) {
        if (g < n) f = mention_flag(s + p);
      } else if (g < n && !is_cont(b)) {
        int len, plen, nlen;
        const uint32_t cp = decode(s + p, &len);
        const bool w = is_word(cp, ascii, table);
        // the preceding code point: its lead is at most 4 bytes back (the halo holds them)
        int q = p - 1;
        while (q > p - 4 && is_cont(s[q])) --q;
        const uint32_t prev = decode(s + q, &plen);
        const bool pw = is_word(prev, ascii, table);
        if (w && !pw) {
          const uint32_t next = decode(s + p + len, &nlen);
          if (is_word(next, ascii, table) && !(lookbehind && (prev == '#' || prev == '@')))
            f = kStart;
        } else if (!w && pw) {
          f = kRunEnd;
        }
        if (b == 0) f |= kNul;
      }
      flags[g] = f;
      my_start += f & kStart;
      my_nul += (f & kNul) ? 1u : 0u;
    }
    // integer adds: the sums do not depend on their order
    my_start = wave_sum(static_cast<int>(my_start));
    my_nul = wave_sum(static_cast<int>(my_nul));
    if ((threadIdx.x & (kWave - 1)) == 0) {
      atomicAdd(&n_start, my_start);
      atomicAdd(&n_nul, my_nul);
    }
    __syncthreads();
    if (threadIdx.x == 0) cnt[tile] = static_cast<u64>(n_start) | (static_cast<u64>(n_nul) << 32);
    __syncthreads();
  }
}

// totals[0] = tokens, totals[1] = NULs, from the exclusive scan of the tiles' counts (n_tiles + 1
// elements, the last count 0).
__global__ void tokenize_totals_kernel(const u64* __restrict__ base, int64_t n_tiles,
                                       int64_t* __restrict__ totals) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const u64 t = base[n_tiles];
  totals[0] = static_cast<int64_t>(t & 0xffffffffull);
  totals[1] = static_cast<int64_t>(t >> 32);
}

// One tile per workgroup, lane t its bytes [16 t, 16 t + 16) in order: token k's start offset,
// and with nul_docs the raw doc_ptr: the document after the k-th NUL begins at the tokens counted
// so far.
__global__ __launch_bounds__(kThreads) void tokenize_spans_kernel(
    int64_t n, const uint8_t* __restrict__ flags, const u64* __restrict__ base, int64_t n_tiles,
    int64_t n_tokens, int64_t* __restrict__ tok_start, int nul_docs, int64_t n_docs,
    int64_t* __restrict__ doc_ptr) {
  typedef hipcub::BlockScan<u64, kThreads> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const int64_t n16 = (n + 15) & ~int64_t{15};
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t g0 = tile * kTile + static_cast<int64_t>(threadIdx.x) * kPerThread;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (g0 < n16) v = *reinterpret_cast<const uint4*>(flags + g0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    u64 mine = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      mine += static_cast<u64>(__popc(w[i] & 0x01010101u)) |
              (static_cast<u64>(__popc(w[i] & 0x04040404u)) << 32);
    u64 before;
    Scan(tmp).ExclusiveSum(mine, before);
    before += base[tile];
    int64_t tok = static_cast<int64_t>(before & 0xffffffffull);
    int64_t nul = static_cast<int64_t>(before >> 32);
#pragma unroll
    for (int i = 0; i < kPerThread; ++i) {
      const uint32_t f = (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
      if (f & kNul) {
        if (nul_docs && nul + 1 < n_docs) doc_ptr[nul + 1] = tok;
        ++nul;
      }
      if (f & kStart) {
        if (tok < n_tokens) tok_start[tok] = g0 + i;
        ++tok;
      }
    }
    __syncthreads();  // tmp is reused by the next tile
  }
  if (nul_docs && blockIdx.x == 0 && threadIdx.x == 0) {
    doc_ptr[0] = 0;
    doc_ptr[n_docs] = n_tokens;
  }
}

// doc_ptr[d] = the number of tokens that start before byte doc_off[d].
__global__ void tokenize_doc_ptr_kernel(int64_t n_docs, const int64_t* __restrict__ doc_off,
                                        int64_t n_tokens, const int64_t* __restrict__ tok_start,
                                        int64_t* __restrict__ doc_ptr) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t d = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= n_docs; d += stride) {
    const int64_t want = doc_off[d];
    int64_t lo = 0, hi = n_tokens;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (tok_start[mid] < want) lo = mid + 1; else hi = mid;
    }
    doc_ptr[d] = lo;
  }
}

__device__ __forceinline__ u64 fmix64(u64 h) {
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
  return h ^ (h >> 33);
}

// A byte as the dictionary sees it: with kFold, ASCII A-Z as a-z (no other byte changes, so a
// multi-byte code point stays itself).
template <bool kFold>
__device__ __forceinline__ uint32_t term_byte(uint32_t b) {
  return (kFold && (b - 'A') < 26u) ? b | 0x20u : b;
}

// One lane per token: walk its bytes to the run's end (FNV-1a, then a finaliser so the low bits
// the sort may be cut to depend on every byte).
template <bool kFold>
__global__ void tokenize_hash_kernel(int64_t n, const uint8_t* __restrict__ text,
                                     const uint8_t* __restrict__ flags, int64_t n_tokens,
                                     const int64_t* __restrict__ tok_start, u64 mask,
                                     int32_t* __restrict__ tok_len, u64* __restrict__ hash,
                                     int32_t* __restrict__ idx) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n_tokens; k += stride) {
    const int64_t s = min(max(tok_start[k], int64_t{0}), n - 1);
    int64_t j = s;
    u64 h = 0xcbf29ce484222325ull;
    do {
      h = (h ^ term_byte<kFold>(text[j])) * 0x100000001b3ull;
      ++j;
    } while (j < n && !(flags[j] & kRunEnd) && j - s < INT32_MAX);
    tok_len[k] = static_cast<int32_t>(j - s);
    hash[k] = fmix64(h) & mask;
    idx[k] = static_cast<int32_t>(k);
  }
}

// head[j] = j where sorted position j opens a run of equal hashes, else 0: an inclusive maximum
// scan turns it into every position's run head.
__global__ void tokenize_heads_kernel(int64_t n_tokens, const u64* __restrict__ key,
                                      int32_t* __restrict__ head) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n_tokens; j += stride)
    head[j] = (j > 0 && key[j] != key[j - 1]) ? static_cast<int32_t>(j) : 0;
}

// Sorted position j: its token against the run's first token (the sort is stable, so that is the
// term's first occurrence), byte by byte (as the hash saw them: folded with kFold). Different
// bytes under one hash set *collision.
template <bool kFold>
__global__ void tokenize_verify_kernel(int64_t n_tokens, const uint8_t* __restrict__ text,
                                       const int64_t* __restrict__ tok_start,
                                       const int32_t* __restrict__ tok_len,
                                       const int32_t* __restrict__ idx,
                                       const int32_t* __restrict__ head,
                                       int32_t* __restrict__ rep_tok, int32_t* __restrict__ is_first,
                                       int32_t* __restrict__ collision) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t j = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n_tokens; j += stride) {
    const int32_t t = idx[j], r = idx[head[j]];
    rep_tok[t] = r;
    is_first[t] = t == r;
    if (t == r) continue;
    const int32_t len = tok_len[t];
    bool same = len == tok_len[r];
    const uint8_t* a = text + tok_start[t];
    const uint8_t* b = text + tok_start[r];
    for (int32_t i = 0; same && i < len; ++i)
      same = term_byte<kFold>(a[i]) == term_byte<kFold>(b[i]);
    if (!same) atomicOr(collision, 1);
  }
}

// Token t's term is its representative's first-appearance number; the terms' spans.
__global__ void tokenize_number_kernel(int64_t n_tokens, const int64_t* __restrict__ tok_start,
                                       const int32_t* __restrict__ tok_len,
                                       const int32_t* __restrict__ rep_tok,
                                       const int32_t* __restrict__ is_first,
                                       const int32_t* __restrict__ first_id,
                                       int32_t* __restrict__ tok_term,
                                       int64_t* __restrict__ term_start,
                                       int32_t* __restrict__ term_len, int64_t* __restrict__ result) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_tokens; t += stride) {
    tok_term[t] = first_id[rep_tok[t]];
    if (is_first[t]) {
      term_start[first_id[t]] = tok_start[t];
      term_len[first_id[t]] = tok_len[t];
    }
    if (t == n_tokens - 1) result[0] = static_cast<int64_t>(first_id[t]) + is_first[t];
  }
}

constexpr int32_t kDrop = GCG_TOKENIZE_DROP;

__global__ void tokenize_keep_kernel(int64_t n_tokens, const int32_t* __restrict__ tok_term,
                                     int64_t n_terms, const int32_t* __restrict__ action,
                                     int32_t* __restrict__ keep) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t <= n_tokens; t += stride) {
    int32_t k = 0;
    if (t < n_tokens) {
      const int32_t term = tok_term[t];
      k = term >= 0 && term < n_terms && action[term] != kDrop;
    }
    keep[t] = k;
  }
}

__global__ void tokenize_remap_kernel(int64_t n_tokens, const int32_t* __restrict__ tok_term,
                                      const int32_t* __restrict__ action,
                                      const int32_t* __restrict__ keep,
                                      const int32_t* __restrict__ pos, int32_t* __restrict__ tokens,
                                      int64_t n_docs, const int64_t* __restrict__ doc_ptr_in,
                                      int64_t* __restrict__ doc_ptr) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (int64_t t = first; t < n_tokens; t += stride)
    if (keep[t]) tokens[pos[t]] = action[tok_term[t]];
  for (int64_t d = first; d <= n_docs; d += stride)
    doc_ptr[d] = pos[min(max(doc_ptr_in[d], int64_t{0}), n_tokens)];
}

int64_t tiles_of(int64_t n_bytes) { return (n_bytes + kTile - 1) / kTile; }

int tile_grid(int64_t n_tiles) {
  return static_cast<int>(std::min<int64_t>(std::max<int64_t>(n_tiles, 1), 1 << 16));
}

// Every space below: the arguments, then the fixed arrays in the order of the take calls (no HIP
// device), then with `sized` the hipcub temporary -- rocPRIM sizes it for the device's
// architecture, so that half needs a HIP device. take_exact throughout: no tokens, empty arrays.

// The scratch of the marking: the tiles' packed counts (and a total), hipcub's temporary.
struct MarkSpace {
  u64* cnt;
  Tmp tmp;
  size_t total;
};

gcg_status mark_space(const char* fn, int64_t n_bytes, void* workspace, bool sized, MarkSpace* s) {
  // a token takes at least three bytes with its separator: below 2^33 bytes the token count
  // fits the low half of a tile's packed count
  if (n_bytes < 0 || n_bytes > (int64_t{1} << 33))
    return fail(GCG_ERR_INVALID_ARG, "%s: bad n_bytes=%lld (at most 2^33)", fn,
                static_cast<long long>(n_bytes));
  Carver cv(workspace);
  s->cnt = cv.take_exact<u64>(tiles_of(n_bytes) + 1);
  TmpSize ts;
  if (sized) {
    ts.add(GCG_CUB(DeviceScan::ExclusiveSum, s->cnt, s->cnt, static_cast<int>(tiles_of(n_bytes) + 1)));
  }
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

// The scratch of the term dictionary.
struct TermsSpace {
  u64 *key_a, *key_b;        // hashes, sorted hashes
  int64_t* tok_start;
  int32_t *idx_a, *idx_b;    // token indices, sorted indices
  int32_t *tok_len, *head, *rep_tok, *is_first, *first_id;
  Tmp tmp;
  size_t total;
};

gcg_status terms_space(const char* fn, int64_t n_tokens, int hash_bits, void* workspace, bool sized,
                       TermsSpace* s) {
  if (n_tokens < 0 || n_tokens >= INT32_MAX || hash_bits < 1 || hash_bits > 64)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad n_tokens=%lld (below 2^31 - 1) or hash_bits=%d "
                "(1 .. 64)", fn, static_cast<long long>(n_tokens), hash_bits);
  Carver cv(workspace);
  s->key_a = cv.take_exact<u64>(n_tokens);
  s->key_b = cv.take_exact<u64>(n_tokens);
  s->tok_start = cv.take_exact<int64_t>(n_tokens);
  s->idx_a = cv.take_exact<int32_t>(n_tokens);
  s->idx_b = cv.take_exact<int32_t>(n_tokens);
  s->tok_len = cv.take_exact<int32_t>(n_tokens);
  s->head = cv.take_exact<int32_t>(n_tokens);
  s->rep_tok = cv.take_exact<int32_t>(n_tokens);
  s->is_first = cv.take_exact<int32_t>(n_tokens);
  s->first_id = cv.take_exact<int32_t>(n_tokens);
  const int n = static_cast<int>(std::max<int64_t>(n_tokens, 1));
  TmpSize ts;
  if (sized) {
    ts.add(GCG_CUB(DeviceRadixSort::SortPairs, s->key_a, s->key_b, s->idx_a, s->idx_b, n, 0, hash_bits));
    ts.add(GCG_CUB(DeviceScan::InclusiveScan, s->idx_a, s->head, hipcub::Max(), n));
    ts.add(GCG_CUB(DeviceScan::ExclusiveSum, s->is_first, s->first_id, n));
  }
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

// The scratch of the remap: the keep flags (n_tokens + 1), their exclusive sum, hipcub's.
struct RemapSpace {
  int32_t *keep, *pos;
  Tmp tmp;
  size_t total;
};

gcg_status remap_space(const char* fn, int64_t n_tokens, int64_t n_docs, int64_t n_terms,
                       void* workspace, bool sized, RemapSpace* s) {
  if (n_tokens < 0 || n_tokens >= INT32_MAX - 1 || n_docs < 0 || n_docs >= INT32_MAX ||
      n_terms < 0 || n_terms > n_tokens)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes n_tokens=%lld n_docs=%lld n_terms=%lld", fn,
                static_cast<long long>(n_tokens), static_cast<long long>(n_docs),
                static_cast<long long>(n_terms));
  Carver cv(workspace);
  s->keep = cv.take_exact<int32_t>(n_tokens + 1);
  s->pos = cv.take_exact<int32_t>(n_tokens + 1);
  TmpSize ts;
  if (sized) {
    ts.add(GCG_CUB(DeviceScan::ExclusiveSum, s->keep, s->pos, static_cast<int>(n_tokens + 1)));
  }
  return ts.take_exact(fn, cv, &s->tmp, &s->total);
}

gcg_status mark_bytes(const char* fn, int64_t n_bytes, size_t* bytes) {
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = 0;
  MarkSpace s;
  if (const gcg_status st = mark_space(fn, n_bytes, nullptr, true, &s)) return st;
  *bytes = s.total;
  return GCG_OK;
}

// The marking under either rule: word runs by `word_table` and `lookbehind`, or with `mentions`
// the mention rule, which takes neither.
gcg_status mark(const char* fn, bool mentions, int64_t n_bytes, const uint8_t* text,
                const uint32_t* word_table, int32_t lookbehind, uint8_t* flags, uint64_t* tile_base,
                int64_t* totals_dev, void* workspace, size_t workspace_bytes, gcg_stream_t stream) {
  MarkSpace s;
  if (const gcg_status st = mark_space(fn, n_bytes, nullptr, false, &s)) return st;
  if ((!mentions && word_table == nullptr) || tile_base == nullptr || totals_dev == nullptr ||
      workspace == nullptr || (n_bytes > 0 && (text == nullptr || flags == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL text, word_table, flags, tile_base, totals_dev or "
                "workspace", fn);
  if (!aligned(text, 16) || !aligned(flags, 16) || !aligned(word_table, 4) ||
      !aligned(tile_base, 8) || !aligned(totals_dev, 8) || !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: text and flags must be 16-byte aligned, the other "
                "buffers to their element size", fn);
  // from here on a HIP device
  if (const gcg_status st = mark_space(fn, n_bytes, workspace, true, &s)) return st;
  if (const gcg_status st = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return st;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n_tiles = tiles_of(n_bytes);
  GCG_HIP_CHECK(hipMemsetAsync(s.cnt + n_tiles, 0, 8, st));
  if (n_tiles > 0) {
    hipLaunchKernelGGL(mentions ? tokenize_mark_kernel<true> : tokenize_mark_kernel<false>,
                       dim3(tile_grid(n_tiles)), dim3(kThreads), 0, st, n_bytes, text, word_table,
                       lookbehind != 0, flags, s.cnt, n_tiles);
    GCG_HIP_CHECK(hipGetLastError());
  }
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, s.cnt, reinterpret_cast<u64*>(tile_base),
      static_cast<int>(n_tiles + 1), st)));
  hipLaunchKernelGGL(tokenize_totals_kernel, dim3(1), dim3(kWave), 0, st,
                     reinterpret_cast<const u64*>(tile_base), n_tiles, totals_dev);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

// The term dictionary; with `fold` A-Z and a-z are one byte to the hash and the comparison.
gcg_status terms(const char* fn, bool fold, int64_t n_bytes, const uint8_t* text,
                 const uint8_t* flags, const uint64_t* tile_base, int64_t n_tokens, int64_t n_docs,
                 const int64_t* doc_off, int32_t hash_bits, int64_t* doc_ptr, int32_t* tok_term,
                 int64_t* term_start, int32_t* term_len, int64_t* result_dev, void* workspace,
                 size_t workspace_bytes, gcg_stream_t stream) {
  TermsSpace s;
  if (const gcg_status st = terms_space(fn, n_tokens, hash_bits, nullptr, false, &s)) return st;
  if (n_bytes < 0 || n_bytes > (int64_t{1} << 33) || n_docs < 1 || n_docs >= INT32_MAX)
    return fail(GCG_ERR_INVALID_ARG, "%s: bad sizes n_bytes=%lld (at most 2^33) n_docs=%lld (at "
                "least one document)", fn, static_cast<long long>(n_bytes),
                static_cast<long long>(n_docs));
  if (n_tokens > n_bytes / 2)
    return fail(GCG_ERR_INVALID_ARG, "%s: %lld tokens do not fit %lld bytes", fn,
                static_cast<long long>(n_tokens), static_cast<long long>(n_bytes));
  if (doc_ptr == nullptr || result_dev == nullptr || tile_base == nullptr ||
      (n_bytes > 0 && (text == nullptr || flags == nullptr)) ||
      (n_tokens > 0 && (tok_term == nullptr || term_start == nullptr || term_len == nullptr ||
                        workspace == nullptr)))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL text, flags, tile_base, doc_ptr, tok_term, "
                "term_start, term_len, result_dev or workspace", fn);
  if (!aligned(flags, 16) || !aligned(tile_base, 8) || !aligned(doc_off, 8) || !aligned(doc_ptr, 8) ||
      !aligned(tok_term, 4) || !aligned(term_start, 8) || !aligned(term_len, 4) ||
      !aligned(result_dev, 8) || !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: flags must be 16-byte aligned, the other buffers to "
                "their element size", fn);
  if (const gcg_status st = terms_space(fn, n_tokens, hash_bits, workspace, true, &s)) return st;
  if (n_tokens > 0)  // no token: no scratch, and the workspace may be NULL
    if (const gcg_status st = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return st;
  hipStream_t st = static_cast<hipStream_t>(stream);
  GCG_HIP_CHECK(hipMemsetAsync(result_dev, 0, 16, st));
  if (n_tokens == 0) {
    GCG_HIP_CHECK(hipMemsetAsync(doc_ptr, 0, static_cast<size_t>(n_docs + 1) * 8, st));
    return GCG_OK;
  }
  const int n = static_cast<int>(n_tokens);
  const int64_t n_tiles = tiles_of(n_bytes);
  const int nul_docs = doc_off == nullptr;
  hipLaunchKernelGGL(tokenize_spans_kernel, dim3(tile_grid(n_tiles)), dim3(kThreads), 0, st, n_bytes,
                     flags, reinterpret_cast<const u64*>(tile_base), n_tiles, n_tokens, s.tok_start,
                     nul_docs, n_docs, doc_ptr);
  GCG_HIP_CHECK(hipGetLastError());
  if (!nul_docs) {
    hipLaunchKernelGGL(tokenize_doc_ptr_kernel, dim3(grid_for(n_docs + 1)), dim3(256), 0, st, n_docs,
                       doc_off, n_tokens, s.tok_start, doc_ptr);
    GCG_HIP_CHECK(hipGetLastError());
  }
  const u64 mask = hash_bits >= 64 ? ~u64{0} : ((u64{1} << hash_bits) - 1);
  hipLaunchKernelGGL(fold ? tokenize_hash_kernel<true> : tokenize_hash_kernel<false>,
                     dim3(grid_for(n_tokens)), dim3(256), 0, st, n_bytes, text, flags, n_tokens,
                     s.tok_start, mask, s.tok_len, s.key_a, s.idx_a);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceRadixSort::SortPairs, s.key_a, s.key_b, s.idx_a, s.idx_b, n, 0,
      static_cast<int>(hash_bits), st)));
  hipLaunchKernelGGL(tokenize_heads_kernel, dim3(grid_for(n_tokens)), dim3(256), 0, st, n_tokens,
                     s.key_b, s.idx_a);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::InclusiveScan, s.idx_a, s.head, hipcub::Max(), n, st)));
  hipLaunchKernelGGL(fold ? tokenize_verify_kernel<true> : tokenize_verify_kernel<false>,
                     dim3(grid_for(n_tokens)), dim3(256), 0, st, n_tokens, text, s.tok_start,
                     s.tok_len, s.idx_b, s.head, s.rep_tok, s.is_first,
                     reinterpret_cast<int32_t*>(result_dev + 1));
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, s.is_first, s.first_id, n, st)));
  hipLaunchKernelGGL(tokenize_number_kernel, dim3(grid_for(n_tokens)), dim3(256), 0, st, n_tokens,
                     s.tok_start, s.tok_len, s.rep_tok, s.is_first, s.first_id, tok_term, term_start, term_len,
                     result_dev);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // namespace

extern "C" {

int32_t gcg_tokenize_tile_bytes(void) { return kTile; }

gcg_status gcg_tokenize_mark_workspace_bytes(int64_t n_bytes, size_t* bytes) {
  return mark_bytes("gcg_tokenize_mark_workspace_bytes", n_bytes, bytes);
}

gcg_status gcg_tokenize_mark(int64_t n_bytes, const uint8_t* text, const uint32_t* word_table,
                             int32_t lookbehind, uint8_t* flags, uint64_t* tile_base,
                             int64_t* totals_dev, void* workspace, size_t workspace_bytes,
                             gcg_stream_t stream) {
  return mark("gcg_tokenize_mark", false, n_bytes, text, word_table, lookbehind, flags, tile_base,
              totals_dev, workspace, workspace_bytes, stream);
}

gcg_status gcg_mention_mark_workspace_bytes(int64_t n_bytes, size_t* bytes) {
  return mark_bytes("gcg_mention_mark_workspace_bytes", n_bytes, bytes);
}

gcg_status gcg_mention_mark(int64_t n_bytes, const uint8_t* text, uint8_t* flags,
                            uint64_t* tile_base, int64_t* totals_dev, void* workspace,
                            size_t workspace_bytes, gcg_stream_t stream) {
  return mark("gcg_mention_mark", true, n_bytes, text, nullptr, 0, flags, tile_base, totals_dev,
              workspace, workspace_bytes, stream);
}

gcg_status gcg_tokenize_terms_workspace_bytes(int64_t n_tokens, int32_t hash_bits, size_t* bytes) {
  const char* fn = "gcg_tokenize_terms_workspace_bytes";
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = 0;
  TermsSpace s;
  if (const gcg_status st = terms_space(fn, n_tokens, hash_bits, nullptr, true, &s)) return st;
  *bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_tokenize_terms(int64_t n_bytes, const uint8_t* text, const uint8_t* flags,
                              const uint64_t* tile_base, int64_t n_tokens, int64_t n_docs,
                              const int64_t* doc_off, int32_t hash_bits, int64_t* doc_ptr,
                              int32_t* tok_term, int64_t* term_start, int32_t* term_len,
                              int64_t* result_dev, void* workspace, size_t workspace_bytes,
                              gcg_stream_t stream) {
  return terms("gcg_tokenize_terms", false, n_bytes, text, flags, tile_base, n_tokens, n_docs,
               doc_off, hash_bits, doc_ptr, tok_term, term_start, term_len, result_dev, workspace,
               workspace_bytes, stream);
}

gcg_status gcg_tokenize_terms_folded(int64_t n_bytes, const uint8_t* text, const uint8_t* flags,
                                     const uint64_t* tile_base, int64_t n_tokens, int64_t n_docs,
                                     const int64_t* doc_off, int32_t hash_bits, int32_t fold_ascii,
                                     int64_t* doc_ptr, int32_t* tok_term, int64_t* term_start,
                                     int32_t* term_len, int64_t* result_dev, void* workspace,
                                     size_t workspace_bytes, gcg_stream_t stream) {
  return terms("gcg_tokenize_terms_folded", fold_ascii != 0, n_bytes, text, flags, tile_base,
               n_tokens, n_docs, doc_off, hash_bits, doc_ptr, tok_term, term_start, term_len,
               result_dev, workspace, workspace_bytes, stream);
}

gcg_status gcg_tokenize_remap_workspace_bytes(int64_t n_tokens, size_t* bytes) {
  const char* fn = "gcg_tokenize_remap_workspace_bytes";
  if (bytes == nullptr) return fail(GCG_ERR_INVALID_ARG, "%s: NULL bytes", fn);
  *bytes = 0;
  RemapSpace s;
  if (const gcg_status st = remap_space(fn, n_tokens, 0, 0, nullptr, true, &s)) return st;
  *bytes = s.total;
  return GCG_OK;
}

gcg_status gcg_tokenize_remap(int64_t n_tokens, const int32_t* tok_term, int64_t n_terms,
                              const int32_t* action, int64_t n_docs, const int64_t* doc_ptr_in,
                              int32_t* tokens, int64_t* doc_ptr, void* workspace,
                              size_t workspace_bytes, gcg_stream_t stream) {
  const char* fn = "gcg_tokenize_remap";
  RemapSpace s;
  if (const gcg_status st = remap_space(fn, n_tokens, n_docs, n_terms, nullptr, false, &s)) return st;
  if (doc_ptr_in == nullptr || doc_ptr == nullptr || workspace == nullptr ||
      (n_tokens > 0 && (tok_term == nullptr || tokens == nullptr)) ||
      (n_terms > 0 && action == nullptr))
    return fail(GCG_ERR_INVALID_ARG, "%s: NULL tok_term, action, doc_ptr_in, tokens, doc_ptr or "
                "workspace", fn);
  if (!aligned(tok_term, 4) || !aligned(action, 4) || !aligned(tokens, 4) ||
      !aligned(doc_ptr_in, 8) || !aligned(doc_ptr, 8) || !aligned(workspace, 8))
    return fail(GCG_ERR_MISALIGNED, "%s: a buffer is not aligned to its element size", fn);
  if (const gcg_status st = remap_space(fn, n_tokens, n_docs, n_terms, workspace, true, &s))
    return st;
  if (const gcg_status st = check_workspace(fn, workspace, workspace_bytes, s.total, 8)) return st;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tokenize_keep_kernel, dim3(grid_for(n_tokens + 1)), dim3(256), 0, st, n_tokens,
                     tok_term, n_terms, action, s.keep);
  GCG_HIP_CHECK(hipGetLastError());
  GCG_HIP_CHECK(s.tmp.run(GCG_CUB(DeviceScan::ExclusiveSum, s.keep, s.pos, static_cast<int>(n_tokens + 1),
      st)));
  hipLaunchKernelGGL(tokenize_remap_kernel, dim3(grid_for(std::max(n_tokens, n_docs + 1))),
                     dim3(256), 0, st, n_tokens, tok_term, action, s.keep, s.pos, tokens, n_docs,
                     doc_ptr_in, doc_ptr);
  GCG_HIP_CHECK(hipGetLastError());
  return GCG_OK;
}

}  // extern "C"
