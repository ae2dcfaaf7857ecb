// lcp_encoder.hip - the reference's breakout encoder on the device: frames -> paddle, blocks and ball of every scene, one launch.
//
// What extract_params (experiments/breakout/encoder.py:63-133, with remove_rect :136-137 and get_pos_dims :140-145) reads off an
// Atari Breakout frame, restated over masks so that it needs no copy of the frame: the reference paints what it has found black
// and searches again; here a pixel is "removed" when it lies in the paddle's rect, a LISTED run's rect or the erase rect.  Only
// channel 0 is read (`frame[..., 0]`): one byte plane k(i, j) = frame[b stride_b + i stride_row + j stride_col].
//   paddle (:67-82)   px = first column of the maximum of row paddle_line; if k(paddle_line, px + ball_w + 1) != paddle_key, the
//                     first column of the maximum of the row from there on; r = first column >= px that is not paddle_key (none,
//                     or r == px: W), at most px + paddle_w
//   blocks (:91-101)  per band i the maximal runs of k(top_i, .) == row_key[i]; a run at column 0 ends the row's list before it
//                     (`while left > 0`); a run that reaches column W - 1 (the reference never returns) ends it too
//   ball (:107-121)   the first pixel in raster order that equals ball_key and is not removed; its extent to the right and downward
//
// One workgroup of four wavefronts per scene.  Rows are staged in LDS by whole 16-byte lines (stride_col <= 4: a lane loads an
// aligned uint4; the first and last line of a row, where the row does not fill them, in at most four aligned pieces, so nothing
// outside the row's own first .. last key byte is read) or, for any other stride, gathered.  The paddle line and the bands' top lines: one wavefront per
// line, 64 columns per pass, `__ballot` masks kept as W-bit rows in LDS - run starts are m & ~((m << 1) | carry).  The ball: the
// frame in blocks of rows; while a lane still holds its 16-byte line it tests the line's key bytes against ball_key four at a time
// (a superset: a row without a candidate is skipped), then a wavefront per candidate row, 64 columns per pass, the removal test
// being rectangle arithmetic plus the band's listed-run mask; the first hit is the minimum linear index (ballot, then one LDS
// minimum) and the workgroup leaves after the first block with a hit.  All LDS is dynamic, so that the staged rows start on a
// 16-byte boundary whatever the tables beside them take.
// Plain stores for every output, no global atomics: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lcp_kernels.h"

namespace lcp {
namespace encoder {

constexpr int EN_T = 256;                  // threads per workgroup (four wavefronts)
constexpr int EN_WAVES = EN_T / 64;
constexpr int MAXROWS = 8;                 // bands
constexpr int MAXWORDS = 16;               // 64-bit words of a W-bit row (W <= 1024)
constexpr int SCAN_BYTES = 16384;          // LDS of one block of rows of the ball scan
constexpr int SCAN_ROWS = 16;
constexpr int NONE = 0x7fffffff;
// the tables behind the staged rows: the bands' listed-run masks, then the ints of `Tables`
constexpr int MASK_BYTES = MAXROWS * MAXWORDS * 8;
constexpr int TABLE_BYTES = MASK_BYTES + 256;

struct Tables {
  int mis[SCAN_ROWS];                      // where column 0 lies in a staged row
  int cand[SCAN_ROWS];                     // ball scan: the staged row may hold ball_key
  int cnt[MAXROWS], st[MAXROWS + 1], pad[2], first, ext[2];
};
static_assert(sizeof(Tables) <= 256 && SCAN_ROWS >= MAXROWS + 1, "the tables of lcp_extract_params_kernel");

// include/lcp_hip.h: the LCP_ENC_LAYOUT_WORDS words, in this order
struct Layout {
  int paddle_line, paddle_h, paddle_w, paddle_key, ball_w, nrows, band_top, band_h;
  int row_key[MAXROWS];
  int er_top, er_left, er_bottom, er_right;
  int ball_key;
};
static_assert(sizeof(Layout) == LCP_ENC_LAYOUT_WORDS * sizeof(int32_t), "the layout words of include/lcp_hip.h");

struct Plane {
  const uint8_t* frame;
  long long sb, sr, sc;                    // bytes between scenes, rows, columns
  int H, W;
  int fast;                                // rows staged by 16-byte lines (sc <= 4), else gathered
  int pitch;                               // bytes of a staged row (a multiple of 16)
  int sce;                                 // bytes between columns of a STAGED row: sc, or 1 when gathered
  int scan_rows;                           // rows per block of the ball scan
  int rows_bytes;                          // LDS of the staged rows; the tables follow
  unsigned nck_inv;                        // 2^24 / (lines of a staged row) + 1: t / lines as a multiplication
};

struct Out {
  int32_t *paddle, *blocks, *nblocks, *ball, *status;
  double *paddle_params, *block_params, *ball_params;
};

// What the listing left in LDS for the ball's removal test.
struct Found {
  int px, pr;                              // the paddle's removed columns px .. pr (inclusive)
  const unsigned long long* mask;          // [MAXROWS][MAXWORDS]: the listed runs of each band
};

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
  const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// bits 0 .. top (top in 0 .. 63)
__device__ __forceinline__ unsigned long long low_bits(int top) { return top >= 63 ? ~0ull : (1ull << (top + 1)) - 1; }

// 0x80 in every byte of w that equals the byte repeated in `rep`, and possibly in bytes above such a byte: never fewer
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t rep) {
  const uint32_t x = w ^ rep;
  return (x - 0x01010101u) & ~x & 0x80808080u;
}
// bits 0 .. 3 of n spread to bit 7 of bytes 0 .. 3
__device__ __forceinline__ uint32_t spread4(uint32_t n) { return (((n & 15u) * 0x00204081u) & 0x01010101u) << 7; }

// A row's first or last line, where the row does not fill it: bytes lo .. hi-1 of the aligned line at `line`, in the largest aligned
// pieces (at most four loads when one end is cut), the rest of the line zero.
__device__ __forceinline__ uint4 load_partial(const uint8_t* line, int lo, int hi) {
  unsigned long long w0 = 0ull, w1 = 0ull;
  auto put = [&](unsigned long long val, int pos) {
    if (pos < 8) w0 |= val << (8 * pos);
    else w1 |= val << (8 * (pos - 8));
  };
  if (lo == 0) {                                                     // the last line: 8, 4, 2, 1 bytes from its start
    int pos = 0;
    if (hi & 8) { put(*reinterpret_cast<const unsigned long long*>(line), 0); pos = 8; }
    if (hi & 4) { put(*reinterpret_cast<const uint32_t*>(line + pos), pos); pos += 4; }
    if (hi & 2) { put(*reinterpret_cast<const uint16_t*>(line + pos), pos); pos += 2; }
    if (hi & 1) put(line[pos], pos);
  } else if (hi == 16) {                                             // the first line: 1, 2, 4, 8 bytes up to its end
    int pos = lo;
    if (pos & 1) { put(line[pos], pos); pos += 1; }
    if (pos & 2) { put(*reinterpret_cast<const uint16_t*>(line + pos), pos); pos += 2; }
    if (pos & 4) { put(*reinterpret_cast<const uint32_t*>(line + pos), pos); pos += 4; }
    if (pos & 8) put(*reinterpret_cast<const unsigned long long*>(line + pos), pos);
  } else {                                                           // a row inside one line
    for (int k = lo; k < hi; ++k) put(line[k], k);
  }
  return make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
}

// stage_rows for a column stride of SC <= 4 bytes: whole 16-byte lines, one per lane
template <int SC>
__device__ __forceinline__ void stage_lines(const Plane& P, const uint8_t* plane, int row0, int rstep, int n, int slot0, uint8_t* rows,
                                            int* mis, int* cand, int key) {
  const int nck = P.pitch >> 4;
  const int span = (P.W - 1) * SC + 1;                               // first .. last key byte of a row
  for (int t = threadIdx.x; t < n * nck; t += EN_T) {
    const int r = (int)(((unsigned)t * P.nck_inv) >> 24), c = t - r * nck;        // t / nck (t < 16 nck <= 4112: exact)
    const uint8_t* a = plane + (long long)(row0 + r * rstep) * P.sr;
    const int m = (int)(reinterpret_cast<uintptr_t>(a) & 15);
    const int off = c * 16 - m;                                      // this line's first byte, relative to the row's first key byte
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (off >= 0 && off + 16 <= span) v = *reinterpret_cast<const uint4*>(a + off);
    else if (off + 16 > 0 && off < span) v = load_partial(a + off, max(0, -off), min(16, span - off));      // only the row's own bytes
    *reinterpret_cast<uint4*>(rows + (size_t)(slot0 + r) * P.pitch + c * 16) = v;
    if (c == 0) mis[slot0 + r] = m;
    if (cand) {
      // the line's key bytes: those at row offsets that are multiples of SC (bytes outside the row are 0, and no key is)
      const int rem = (int)((unsigned)(off + 48) % (unsigned)SC);    // (off >= -15; 48 is a multiple of every SC)
      const int k0 = rem ? SC - rem : 0;
      constexpr uint32_t pat = SC == 1 ? 0xffffu : SC == 2 ? 0x5555u : SC == 3 ? 0x9249u : 0x1111u;
      const uint32_t bm = (pat << k0) & 0xffffu;
      const uint32_t kr = (uint32_t)key * 0x01010101u;
      const uint32_t any = (eq_bytes(v.x, kr) & spread4(bm)) | (eq_bytes(v.y, kr) & spread4(bm >> 4)) |
                           (eq_bytes(v.z, kr) & spread4(bm >> 8)) | (eq_bytes(v.w, kr) & spread4(bm >> 12));
      if (any) cand[slot0 + r] = 1;
    }
  }
}

// Rows row0, row0 + rstep, .. (n of them) of the key plane into the staged rows slot0 ..; mis[slot]: where column 0 lies in it.
// cand (or NULL): cand[slot] is set when the row may hold `key` in the key plane (never missed; the caller has zeroed it).
__device__ __forceinline__ void stage_rows(const Plane& P, const uint8_t* plane, int row0, int rstep, int n, int slot0, uint8_t* rows,
                                           int* mis, int* cand = nullptr, int key = 0) {
  if (P.fast) {
    switch (P.sce) {
      case 1: stage_lines<1>(P, plane, row0, rstep, n, slot0, rows, mis, cand, key); break;
      case 2: stage_lines<2>(P, plane, row0, rstep, n, slot0, rows, mis, cand, key); break;
      case 3: stage_lines<3>(P, plane, row0, rstep, n, slot0, rows, mis, cand, key); break;
      default: stage_lines<4>(P, plane, row0, rstep, n, slot0, rows, mis, cand, key); break;
    }
  } else {
    for (int t = threadIdx.x; t < n * P.W; t += EN_T) {
      const int r = t / P.W, j = t - r * P.W;
      const uint8_t v = plane[(long long)(row0 + r * rstep) * P.sr + (long long)j * P.sc];
      rows[(size_t)(slot0 + r) * P.pitch + j] = v;
      if (j == 0) mis[slot0 + r] = 0;
      if (cand && v == key) cand[slot0 + r] = 1;
    }
  }
}

// k(row of `slot`, j) from the staged rows
__device__ __forceinline__ int pix(const Plane& P, const uint8_t* rows, const int* mis, int slot, int j) {
  return rows[(size_t)slot * P.pitch + mis[slot] + j * P.sce];
}

// The first column >= from holding the maximum of the staged row from there on (np.argmax; from < W).
__device__ __forceinline__ int first_max(const Plane& P, const uint8_t* rows, const int* mis, int slot, int from) {
  const int lane = threadIdx.x & 63;
  int bv = -1, bc = NONE;
  for (int j = lane; j < P.W; j += 64) {
    if (j >= from) {
      const int v = pix(P, rows, mis, slot, j);
      if (v > bv) { bv = v; bc = j; }
    }
  }
  const int M = wave_max(bv);
  return wave_min(bv == M ? bc : NONE);
}

// encoder.py:67-82, by one wavefront; returns the status bits
__device__ __forceinline__ int find_paddle(const Plane& P, const Layout& L, const uint8_t* rows, const int* mis, int slot, int* px_out,
                                           int* r_out) {
  const int lane = threadIdx.x & 63, W = P.W;
  int st = 0;
  int px = first_max(P, rows, mis, slot, 0);
  const int probe = px + L.ball_w + 1;
  if (probe >= W) st |= LCP_ENC_ST_PADDLE_PROBE;                      // (the reference raises IndexError)
  else if (pix(P, rows, mis, slot, probe) != L.paddle_key) px = first_max(P, rows, mis, slot, probe);
  int r = W;
  for (int q = px >> 6; q * 64 < W; ++q) {
    const int j = q * 64 + lane;
    const unsigned long long m = __ballot(j >= px && j < W && pix(P, rows, mis, slot, j) != L.paddle_key);
    if (m) { r = q * 64 + __ffsll((long long)m) - 1; break; }
  }
  if (r == px) r = W;                                                // (np.argmin of all-True and of a False first: both 0)
  r = min(r, px + L.paddle_w);
  *px_out = px; *r_out = r;
  return st;
}

// encoder.py:91-101 for band `slot`, by one wavefront: the listed runs as a W-bit mask (lane q returns word q), their number
// in *count; returns the status bits
__device__ __forceinline__ int list_band(const Plane& P, const Layout& L, const uint8_t* rows, const int* mis, int slot,
                                         unsigned long long* word_out, int* count) {
  const int lane = threadIdx.x & 63, W = P.W;
  const int key = L.row_key[slot];
  const int wlast = (W - 1) >> 6;
  unsigned long long mine = 0ull;
  for (int q = 0; q <= wlast; ++q) {
    const int j = q * 64 + lane;
    const unsigned long long m = __ballot(j < W && pix(P, rows, mis, slot, j) == key);
    if (lane == q) mine = m;
  }
  int st = 0;
  const unsigned long long w0 = shfl64(mine, 0), wl = shfl64(mine, wlast);
  if (w0 & 1ull) {
    mine = 0ull;                                                     // `while left > 0`: a run at column 0 ends the list before it
  } else if ((wl >> ((W - 1) & 63)) & 1ull) {
    // the run that reaches column W - 1 is not listed: cleared from the highest zero of the row upward
    st |= LCP_ENC_ST_RUN_AT_EDGE;
    const int top = lane == wlast ? ((W - 1) & 63) : 63;
    const unsigned long long zeros = lane <= wlast ? ~mine & low_bits(top) : 0ull;
    const unsigned long long has = __ballot(zeros != 0ull);          // (bit 0 of word 0 is a zero here: never empty)
    const int qz = 63 - __clzll((long long)has);
    if (lane > qz) mine = 0ull;
    else if (lane == qz) mine &= low_bits(63 - __clzll((long long)zeros));
  }
  unsigned long long prev = shfl64(mine, lane > 0 ? lane - 1 : 0);
  const unsigned long long carry = lane > 0 ? prev >> 63 : 0ull;
  const unsigned long long starts = mine & ~((mine << 1) | carry);
  *count = wave_sum(__popcll(starts));
  *word_out = mine;
  return st;
}

__device__ __forceinline__ bool listed(const Found& F, int band, int j) { return (F.mask[band * MAXWORDS + (j >> 6)] >> (j & 63)) & 1ull; }

// whether the reference has painted pixel (i, j) black before it looks for the ball
__device__ __forceinline__ bool removed(const Layout& L, const Found& F, int i, int j) {
  if (i >= L.paddle_line && i <= L.paddle_line + L.paddle_h && j >= F.px && j <= F.pr) return true;
  if (i >= L.er_top && i <= L.er_bottom && j >= L.er_left && j <= L.er_right) return true;
  const int d = i - L.band_top;
  if (d >= 0 && d < L.nrows * L.band_h) return listed(F, d / L.band_h, j);
  return false;
}

__global__ void __launch_bounds__(EN_T) lcp_extract_params_kernel(Plane P, Layout L, int max_blocks, Out O) {
  extern __shared__ uint4 s_dyn[];                                    // [the staged rows][s_mask][Tables]
  uint8_t* rows = reinterpret_cast<uint8_t*>(s_dyn);
  unsigned long long* s_mask = reinterpret_cast<unsigned long long*>(rows + P.rows_bytes);
  Tables& T = *reinterpret_cast<Tables*>(rows + P.rows_bytes + MASK_BYTES);
  int *s_mis = T.mis, *s_cnt = T.cnt, *s_st = T.st, *s_pad = T.pad, *s_ext = T.ext;
  int& s_first = T.first;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = P.H, W = P.W;
  const size_t b = blockIdx.x;
  const uint8_t* plane = P.frame + (long long)b * P.sb;

  // ---- the paddle line (slot nrows) and the bands' top lines (slots 0 .. nrows-1): one wavefront per line
  stage_rows(P, plane, L.band_top, L.band_h, L.nrows, 0, rows, s_mis);
  stage_rows(P, plane, L.paddle_line, 0, 1, L.nrows, rows, s_mis);
  if (tid == 0) s_first = NONE;
  __syncthreads();
  for (int s = wave; s <= L.nrows; s += EN_WAVES) {
    if (s == L.nrows) {
      int px, r;
      const int st = find_paddle(P, L, rows, s_mis, s, &px, &r);
      if (lane == 0) { s_pad[0] = px; s_pad[1] = r; s_st[MAXROWS] = st; }
    } else {
      unsigned long long word;
      int count;
      const int st = list_band(P, L, rows, s_mis, s, &word, &count);
      if (lane < MAXWORDS) s_mask[s * MAXWORDS + lane] = word;
      if (lane == 0) { s_cnt[s] = count; s_st[s] = st; }
    }
  }
  __syncthreads();
  Found F;
  F.px = s_pad[0]; F.pr = s_pad[1]; F.mask = s_mask;
  int total = 0, status = s_st[MAXROWS];
  for (int s = 0; s < L.nrows; ++s) { total += s_cnt[s]; status |= s_st[s]; }
  if (total > max_blocks) status |= LCP_ENC_ST_TRUNCATED;

  // ---- the block list: row by row, left to right; slots >= the count hold zeros / the reference's placeholder block
  for (int s = wave; s < L.nrows; s += EN_WAVES) {
    int rank0 = 0;
    for (int t = 0; t < s; ++t) rank0 += s_cnt[t];
    const int top = L.band_top + s * L.band_h;
    for (int q = 0; q * 64 < W && rank0 < max_blocks; ++q) {
      const unsigned long long m = s_mask[s * MAXWORDS + q];
      const unsigned long long carry = q > 0 ? s_mask[s * MAXWORDS + q - 1] >> 63 : 0ull;
      const unsigned long long starts = m & ~((m << 1) | carry);
      const int rank = rank0 + __popcll(starts & ((1ull << lane) - 1));
      if (((starts >> lane) & 1ull) && rank < max_blocks) {
        const int left = q * 64 + lane;
        int right = W;
        const unsigned long long z = ~m >> lane;                     // (bit 0: this run's own start, a one of m)
        if (z) {
          right = left + __ffsll((long long)z) - 1;
        } else {
          for (int q2 = q + 1; q2 * 64 < W; ++q2) {
            const unsigned long long z2 = ~s_mask[s * MAXWORDS + q2];
            if (z2) { right = q2 * 64 + __ffsll((long long)z2) - 1; break; }
          }
        }
        const size_t slot = b * max_blocks + rank;
        if (O.blocks) {
          int32_t* c = O.blocks + slot * 4;
          c[0] = top; c[1] = left; c[2] = top + L.band_h; c[3] = right;
        }
        if (O.block_params) {                                        // get_pos_dims, encoder.py:140-145
          double* g = O.block_params + slot * 4;
          g[0] = 0.5 * (right + left); g[1] = 0.5 * (2 * top + L.band_h); g[2] = (double)(right - left); g[3] = (double)L.band_h;
        }
      }
      rank0 += __popcll(starts);
    }
  }
  for (int k = total + tid; k < max_blocks; k += EN_T) {
    const size_t slot = b * max_blocks + k;
    if (O.blocks) { int32_t* c = O.blocks + slot * 4; c[0] = 0; c[1] = 0; c[2] = 0; c[3] = 0; }
    if (O.block_params) { double* g = O.block_params + slot * 4; g[0] = 1000.0; g[1] = 60.0; g[2] = 1.0; g[3] = 1.0; }   // run_breakout.py:56
  }
  if (tid == 0) {
    const int bottom = L.paddle_line + L.paddle_h;
    if (O.nblocks) O.nblocks[b] = total;
    if (O.paddle) { int32_t* c = O.paddle + b * 4; c[0] = L.paddle_line; c[1] = F.px; c[2] = bottom; c[3] = F.pr; }
    if (O.paddle_params) {
      double* g = O.paddle_params + b * 4;
      g[0] = 0.5 * (F.pr + F.px); g[1] = 0.5 * (bottom + L.paddle_line); g[2] = (double)(F.pr - F.px); g[3] = (double)L.paddle_h;
    }
  }
  if (!O.ball && !O.ball_params && !O.status) return;                // (the ball decides NO_BALL: status needs the scan)

  // ---- the ball: the frame in blocks of rows, a wavefront per row, until the first block with a hit
  int i0 = 0;
  for (; i0 < H; i0 += P.scan_rows) {
    const int nr = min(P.scan_rows, H - i0);
    if (tid < SCAN_ROWS) T.cand[tid] = 0;
    __syncthreads();                                                 // (the readers of what `rows` held)
    stage_rows(P, plane, i0, 1, nr, 0, rows, s_mis, T.cand, L.ball_key);
    __syncthreads();
    for (int r = wave; r < nr; r += EN_WAVES) {
      if (!T.cand[r]) continue;                                      // no ball_key in this row's key bytes
      const uint8_t* rp = rows + (size_t)r * P.pitch + s_mis[r];
      const int i = i0 + r;
      const bool in_pad = i >= L.paddle_line && i <= L.paddle_line + L.paddle_h;
      const bool in_er = i >= L.er_top && i <= L.er_bottom;
      const int d = i - L.band_top;
      const int band = d >= 0 && d < L.nrows * L.band_h ? d / L.band_h : -1;
      bool hit = false;
      for (int q = 0; q * 64 < W; ++q) {
        const int j = q * 64 + lane;
        const unsigned long long lw = band >= 0 ? F.mask[band * MAXWORDS + q] : 0ull;
        bool h = j < W && rp[j * P.sce] == L.ball_key && !((lw >> lane) & 1ull);
        if (h && in_pad && j >= F.px && j <= F.pr) h = false;
        if (h && in_er && j >= L.er_left && j <= L.er_right) h = false;
        const unsigned long long m = __ballot(h);
        if (m) {
          if (lane == 0) atomicMin(&s_first, i * W + q * 64 + __ffsll((long long)m) - 1);          // (LDS)
          hit = true;
          break;
        }
      }
      if (hit) break;                                                // (this wavefront's later rows lie behind it)
    }
    __syncthreads();
    if (s_first != NONE) break;
  }
  const int first = s_first;
  const bool found = first != NONE;
  const int bi = found ? first / W : 0, bj = found ? first - bi * W : 0;
  if (found && wave == 0) {
    // to the right in the ball's row, which the last block still holds
    int right = bj;                                                  // (np.argmin of all-True: 0)
    const int r = bi - i0;
    for (int q = bj >> 6; q * 64 < W; ++q) {
      const int j = q * 64 + lane;
      const unsigned long long m = __ballot(j >= bj && j < W && (pix(P, rows, s_mis, r, j) != L.ball_key || removed(L, F, bi, j)));
      if (m) { right = q * 64 + __ffsll((long long)m) - 1; break; }
    }
    if (lane == 0) s_ext[0] = right;
  }
  if (found && wave == 1) {
    // downward in the ball's column: one byte per row, there is no line to share
    int bottom = bi;
    for (int base = bi; base < H; base += 64) {
      const int i = base + lane;
      bool stop = false;
      if (i < H) stop = plane[(long long)i * P.sr + (long long)bj * P.sc] != L.ball_key || removed(L, F, i, bj);
      const unsigned long long m = __ballot(stop);
      if (m) { bottom = base + __ffsll((long long)m) - 1; break; }
    }
    if (lane == 0) s_ext[1] = bottom;
  }
  __syncthreads();
  if (tid == 0) {
    const int right = found ? s_ext[0] : 0, bottom = found ? s_ext[1] : 0;
    if (!found) status |= LCP_ENC_ST_NO_BALL;
    if (O.status) O.status[b] = status;
    if (O.ball) { int32_t* c = O.ball + b * 4; c[0] = bi; c[1] = bj; c[2] = bottom; c[3] = right; }
    if (O.ball_params) {
      double* g = O.ball_params + b * 3;
      if (found) {                                                   // encoder.py:124-125
        const double w = (double)(right - bj), h = (double)(bottom - bi);
        g[0] = 0.5 * (right + bj); g[1] = 0.5 * (bottom + bi); g[2] = fmin(0.5 * fmin(w, h), 1.0);
      } else {                                                       // encoder.py:129: far off, to incur a high cost
        g[0] = 0.5 * W; g[1] = 100.0 * H; g[2] = 1.0;
      }
    }
  }
}

}  // namespace encoder

int extract_params_launch(int B, int H, int W, const uint8_t* frame, long long stride_b, long long stride_row, long long stride_col,
                          const int32_t* layout, int max_blocks, int32_t* paddle, int32_t* blocks, int32_t* nblocks, int32_t* ball,
                          int32_t* status, double* paddle_params, double* block_params, double* ball_params, void* stream) {
  using namespace encoder;
  Layout L;
  int32_t* lw = reinterpret_cast<int32_t*>(&L);
  for (int k = 0; k < LCP_ENC_LAYOUT_WORDS; ++k) lw[k] = layout[k];
  Plane P;
  P.frame = frame; P.sb = stride_b; P.sr = stride_row; P.sc = stride_col; P.H = H; P.W = W;
  P.fast = stride_col <= 4;
  P.sce = P.fast ? (int)stride_col : 1;
  // a row's lines: its first .. last key byte, and one more for a first byte that does not start a line
  P.pitch = P.fast ? (int)((((long long)(W - 1) * stride_col + 1 + 15) / 16 + 1) * 16) : (W + 15) / 16 * 16;
  P.nck_inv = (1u << 24) / (unsigned)(P.pitch >> 4) + 1u;
  int sr = SCAN_BYTES / P.pitch;
  P.scan_rows = sr < 1 ? 1 : sr > SCAN_ROWS ? SCAN_ROWS : sr;
  const int slots = P.scan_rows > L.nrows + 1 ? P.scan_rows : L.nrows + 1;
  P.rows_bytes = slots * P.pitch;                                    // (at most 9 x 4112 B: with the tables < 64 KB)
  const size_t lds = (size_t)P.rows_bytes + TABLE_BYTES;
  Out O{paddle, blocks, nblocks, ball, status, paddle_params, block_params, ball_params};
  void* args[] = {&P, &L, &max_blocks, &O};
  if (hipLaunchKernel(reinterpret_cast<const void*>(lcp_extract_params_kernel), dim3((unsigned)B), dim3(EN_T), args, lds,
                      (hipStream_t)stream) != hipSuccess)
    return LCP_E_LAUNCH;
  return hipGetLastError() == hipSuccess ? 0 : LCP_E_LAUNCH;
}

}  // namespace lcp
