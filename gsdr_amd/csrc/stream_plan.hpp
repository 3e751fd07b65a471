// gsdr-mi355x: what one call of a streaming object does (gsdrxStreamProcess, include/gsdr/stream.h;
// gsdrxResamplerProcess, include/gsdr/resampler.h), as pure functions of the filter's shape and the stream's
// position: which outputs the call writes (stream_plan) and where the kept samples go (the move lists). No HIP, so
// it is compiled and checked on the host alone (gsdrxStreamPlan and gsdrxResamplerPlan expose the plan,
// tests/test_stream_moves.py walks the move lists).
//
// L = interpolation, M = decimation, T = taps >= 1, q = phase0 < L. Output m's window starts at s(m) = q + m M of
// the zero-stuffed stream; it reads the samples [first(m), need(m)) of the stream,
//     first(m) = ceil(s(m) / L),   need(m) = floor((s(m) + T - 1) / L) + 1   (gsdrxResampleInputsFor of m + 1 outputs),
// none when the window holds no tap (first = need), and is written by the first call after which need(m) samples
// have arrived. Both are non-decreasing in m, and need(m) - first(m) <= ceil(T / L). gsdrxStream is L = 1, q = 0,
// M = its decimation and T = the samples one of its outputs needs: first(m) = m M, need(m) = m M + T.
//
// Between calls the object keeps x[first(m) .. consumed) for m = the next output. That output has not been written,
// so need(m) > consumed, hence consumed - first(m) < need(m) - first(m) <= ceil(T / L): the history holds at most
// ceil(T / L) - 1 samples. When M / L is large first(m) may lie beyond consumed: the history is empty and
// first(m) - consumed samples of the coming chunks are skipped.
#pragma once

#include <stdint.h>

namespace gsdr {

struct StreamPlan {
  uint64_t outputs;     // outputs this call writes
  uint64_t seam;        // the first `seam` of them start in the history (first(m) < consumed)
  uint64_t hist;        // history samples in use before the call
  uint64_t skip;        // samples at the head of the chunk that no output reads: min(first(m) - consumed, chunk)
  uint64_t hist_after;  // history samples after the call
  uint64_t skip_after;  // samples of later chunks still to skip after the call
  // for the launches: first(m) of the next output before and after the call
  uint64_t first, first_after;
  // for the seam plan (two one-shot calls; a one-shot call at output m' reads from x[origin(m')], origin = s / L)
  uint64_t lead;     // first - origin of the next output: 0 or 1
  uint64_t head;     // chunk samples the last seam output reads: need(m + seam - 1) - consumed (0: no seam output)
  int64_t main_off;  // origin(m + seam) - consumed: where in the chunk the other outputs' call starts (0: none)
};

typedef unsigned __int128 stream_u128;

// s(m) = q + m M when s(m) + T stays within 63 bits
inline bool stream_stuffed(uint64_t q, uint64_t M, uint64_t T, uint64_t m, uint64_t* s) {
  const stream_u128 v = (stream_u128)m * M + q;
  if (((v + T) >> 63) != 0) return false;
  *s = (uint64_t)v;
  return true;
}

// Outputs whose samples all lie in x[0, S): the m with s(m) + T <= S L, from 0.
inline uint64_t stream_outputs_through(uint64_t L, uint64_t M, uint64_t T, uint64_t q, uint64_t S) {
  const stream_u128 have = (stream_u128)S * L, least = (stream_u128)T + q;
  if (have < least) return 0;
  const stream_u128 n = (have - least) / M + 1;
  return (n >> 64) != 0 ? ~0ull : (uint64_t)n;
}

// The call that appends `chunk` samples to a stream of which `S` have arrived and `m` outputs are written. False:
// refused (a bad shape, or the zero-stuffed index s + T of an output of this call or of the next one leaves 63 bits).
inline bool stream_plan(uint64_t L, uint64_t M, uint64_t T, uint64_t q, uint64_t S, uint64_t m, uint64_t chunk,
                        StreamPlan* p) {
  *p = StreamPlan{};
  uint64_t S1 = 0, s = 0, s_end = 0;
  if (L == 0 || M == 0 || T == 0 || q >= L || __builtin_add_overflow(S, chunk, &S1)) return false;
  uint64_t m_end = stream_outputs_through(L, M, T, q, S1);
  if (m_end < m) m_end = m;
  if (!stream_stuffed(q, M, T, m, &s) || !stream_stuffed(q, M, T, m_end, &s_end)) return false;
  p->outputs = m_end - m;
  p->first = s / L + (s % L != 0);
  p->first_after = s_end / L + (s_end % L != 0);
  // first(m') < S  <=>  s(m') <= (S - 1) L
  uint64_t m_mid = m;
  if (S > 0 && (stream_u128)(S - 1) * L >= q) {
    const stream_u128 n = ((stream_u128)(S - 1) * L - q) / M + 1;
    m_mid = n > m_end ? m_end : (uint64_t)n;
    if (m_mid < m) m_mid = m;
  }
  p->seam = m_mid - m;
  p->hist = S > p->first ? S - p->first : 0;
  p->skip = p->first > S ? (p->first - S < chunk ? p->first - S : chunk) : 0;
  p->hist_after = S1 > p->first_after ? S1 - p->first_after : 0;
  p->skip_after = p->first_after > S1 ? p->first_after - S1 : 0;
  // (m <= m_mid <= m_end: s(m_mid) + T is within 63 bits as s_end + T is)
  const uint64_t s_mid = s + p->seam * M;
  p->lead = p->first - s / L;
  if (p->seam) p->head = (s_mid - M + T - 1) / L + 1 - S;
  if (m_mid < m_end) p->main_off = (int64_t)(s_mid / L - S);
  return true;
}

// ---- where the kept samples go --------------------------------------------------------------------------------
// The small device-to-device moves of one call, in samples, between the object's three buffers and the caller's
// chunk. At most four, none empty; they write the spare history or the seam buffer and read the history in use or
// the chunk, so none overlaps another.
enum StreamBuffer { kHist, kSpare, kSeam, kChunk };

struct StreamMoves {
  static constexpr int kMax = 4;
  struct Seg {
    StreamBuffer dst;
    uint64_t dst_off;
    StreamBuffer src;
    uint64_t src_off, count;
  } seg[kMax];
  int n = 0;
  void add(StreamBuffer dst, uint64_t dst_off, StreamBuffer src, uint64_t src_off, uint64_t count) {
    if (count) seg[n++] = Seg{dst, dst_off, src, src_off, count};
  }
};

// What the lists may use: history and spare hold ceil(T / L) samples (one more than a history ever has), the seam
// buffer lead + history + head <= 1 + 2 (ceil(T / L) - 1) < twice that.
inline uint64_t stream_hist_capacity(uint64_t L, uint64_t T) { return T / L + (T % L != 0); }
inline uint64_t stream_seam_capacity(uint64_t L, uint64_t T) { return 2 * stream_hist_capacity(L, T); }

// The next history x[first_after .. S + chunk) into the spare buffer: the tail of the old history when first_after
// lies in it (then the whole chunk follows), then the tail of the chunk. With d = first_after - first: the old
// history covers d < hist; otherwise the chunk part starts skip + d - hist samples in (hist and skip are never both
// non-zero, and hist_after > 0 means the chunk reaches past first, so skip = first - S in full).
inline void stream_next_history(const StreamPlan& p, uint64_t chunk, StreamMoves* mv) {
  if (p.hist_after == 0) return;
  const uint64_t d = p.first_after - p.first;
  const uint64_t kept = d < p.hist ? p.hist - d : 0;
  const uint64_t c0 = d < p.hist ? 0 : p.skip + d - p.hist;
  mv->add(kSpare, 0, kHist, d, kept);
  mv->add(kSpare, kept, kChunk, c0, chunk - c0);
}

// The seam buffer, whose sample 0 is x[origin] of the next output: the history at `lead`, then the chunk head.
inline void stream_seam(const StreamPlan& p, StreamMoves* mv) {
  if (p.seam == 0) return;
  mv->add(kSeam, p.lead, kHist, 0, p.hist);
  mv->add(kSeam, p.lead + p.hist, kChunk, 0, p.head);
}

}  // namespace gsdr
