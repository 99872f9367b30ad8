// quant_plan.h — host plan of ps_quantize_f32 / ps_dequantize_f32 (host side only, no HIP: plain C++17).
//
// A descriptor list becomes ONE QuantPlan: the tensor table the kernels read, the per-chunk table that maps a
// workgroup to its tensor, and where each launch's list starts in it.  Every non-empty tensor is on exactly one path:
//
//   strip  quantize only.  Contiguous, float4-addressable, 64 ... 4096 rows: strips of QS_COLS columns kept in
//          registers.  More than 1024 rows: `team` parts of 1024 rows per strip, one workgroup each.
//   small  quantize only.  Any layout, up to 1024 rows, not a strip: ranges of small_w columns, ALL rows each.
//   flat   contiguous, float4-addressable, at most QFLAT_MAXC columns and QMAXT elements: chunks of QFLAT
//          consecutive elements (every such tensor on dequantize, those of more than 4096 rows on quantize).
//   tile   everything else (strided views, odd column counts or alignments, huge tensors): QR x QW tiles.
// tests/quant_plan_host.cpp drives this file on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/ps_api.h"

namespace psk {

constexpr int QW = 256;           // tile: columns per chunk
constexpr int QR = 64;            // tile: rows per chunk
constexpr int QFLAT = 16384;      // flat: elements per chunk (16 float4 per thread)
constexpr int QFLAT_MAXC = 8192;  // flat: columns kept in LDS by the column-max pass
constexpr int QMAXT = 1 << 30;    // flat: elements per tensor (32-bit row / column arithmetic)
constexpr int QS_COLS = 64;       // strip: columns per strip
constexpr int QS_THREADS = 512;
constexpr int QS_GROUPS = QS_THREADS / 16;   // 32 row groups
constexpr int QS_NV = 32;                    // rows per lane
constexpr int QS_ROWS = QS_NV * QS_GROUPS;   // 1024 rows per workgroup: a whole strip, or one part of a tall one
constexpr int QS_MAX_TEAM = 4;               // parts per tall strip
constexpr int QS_MINR = 64;                  // below that a strip is too little work per workgroup
constexpr int QSM_ELEMS = 65536;             // small: elements per item
constexpr int QSM_COLS = 2048;               // small: columns per item (LDS)
constexpr int QUEUE_WORDS = 4;               // the strip queue's counter, padded

// quant_strip_kernel addresses a tensor with 32-bit byte offsets: a strip tensor is flat (<= QFLAT_MAXC columns)
// and has at most QS_MAX_TEAM * QS_ROWS rows
static_assert((long long)QS_MAX_TEAM * QS_ROWS * QFLAT_MAXC * 4 < (1LL << 31), "strip tensors: 32-bit byte offsets");
static_assert((long long)QS_MAX_TEAM * QS_ROWS * QFLAT_MAXC <= QMAXT, "every strip candidate passes the flat guard");

enum QPath : int { Q_EMPTY = 0, Q_STRIP, Q_SMALL, Q_FLAT, Q_TILE };

struct QTensor {          // one row of the device's tensor table
  const float* fin;       // quantize input
  float* fout;            // dequantize output (the same buffer: ps_quant_desc::fvalue)
  void* codes;
  float* diag;
  float* bucket;
  unsigned* colmax;       // workspace: bit patterns of the column maxima (quantize only)
  unsigned* sarrive;      // workspace: per strip of a team, the parts whose column maxima are merged
  long long rows, cols, ld, ldq;
  int bits, extract;
  int path;               // QPath
  int vec4;               // tile: the float4 branch
  int chunk0, chunks;     // the tensor's items in the list of its path: first one, how many
  int strips;             // tile: column strips of QW columns (chunk = row chunk * strips + strip)
  int team;               // strip: parts of QS_ROWS rows per strip (1 = whole strips)
  int small_w;            // small: columns per item
};

inline size_t quant_pad4(size_t c) { return (c + 3) / 4 * 4; }   // a tensor's column maxima: whole uint4s

struct QuantPlan {
  std::vector<QTensor> tensors;
  // one word (tensor index) per flat chunk, tile chunk and strip item, then two words (tensor index, first column)
  // per small item
  std::vector<int> table;
  int flat_chunks = 0, tile_chunks = 0, strip_items = 0, small_items = 0;
  size_t flat_off = 0, tile_off = 0, strip_off = 0, small_off = 0;   // first word of each list in `table`
  // quantize scratch (one memset): column maxima of every tensor | the strip queue's counter | one arrival counter
  // per strip of a team
  size_t total_cols = 0, team_strips = 0;
  size_t queue_off() const { return total_cols; }
  size_t scratch_words() const { return total_cols + QUEUE_WORDS + team_strips; }

  // points every tensor at its part of the scratch
  void bind_scratch(unsigned* scratch) {
    size_t off = 0, soff = total_cols + QUEUE_WORDS;
    for (QTensor& t : tensors) {
      t.colmax = scratch + off;
      off += quant_pad4((size_t)t.cols);
      if (t.team > 1) { t.sarrive = scratch + soff; soff += (size_t)(t.chunks / t.team); }
    }
  }
};

inline bool quant_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// Upper bounds for the workspace queries, which see the descriptors but build no plan: words of the per-chunk
// table (a tensor is in one list; the last term covers small items: one per range of >= 64 columns, or one in
// all) and words of the quantize scratch.
inline size_t quant_table_bound(const ps_quant_desc* desc, int count) {
  size_t n = 0;
  for (int i = 0; i < count; ++i) {
    const long long rows = desc[i].rows, cols = desc[i].cols;
    if (rows <= 0 || cols <= 0) continue;
    const size_t flat = (size_t)((rows * cols + QFLAT - 1) / QFLAT);
    const size_t tile = (size_t)((cols + QW - 1) / QW) * (size_t)((rows + QR - 1) / QR);
    const size_t strips = (size_t)QS_MAX_TEAM * (size_t)((cols + QS_COLS - 1) / QS_COLS);
    n += std::max(std::max(flat, tile), strips) + 2 * ((size_t)cols / 64 + 1);
  }
  return n;
}
inline size_t quant_scratch_bound(const ps_quant_desc* desc, int count) {
  size_t n = QUEUE_WORDS;
  for (int i = 0; i < count; ++i) {
    const size_t c = (size_t)(desc[i].cols > 0 ? desc[i].cols : 0);
    n += quant_pad4(c) + (c + QS_COLS - 1) / QS_COLS;
  }
  return n;
}

// Validates, classifies and lays out in one pass over the descriptors.  PS_OK, or the refusal.
inline int quant_build_plan(const ps_quant_desc* desc, int count, bool encode, QuantPlan& p) {
  p = QuantPlan();
  p.tensors.resize((size_t)count);
  long long n_flat = 0, n_tile = 0, n_strip = 0, n_small = 0;
  long long as_tiles = 0;   // the list as tile chunks: the size limit of a call
  for (int i = 0; i < count; ++i) {
    const ps_quant_desc& d = desc[i];
    if (d.rows < 0 || d.cols < 0 || (d.bits != 8 && d.bits != 16)) return PS_EINVAL;
    const bool nonempty = d.rows > 0 && d.cols > 0;
    if (nonempty) {
      if (!d.fvalue || !d.codes || !d.bucket_size || d.ld < d.cols || d.ldq < d.cols) return PS_EINVAL;
      if (d.extract_diagonal && (!d.diagonal || d.rows != d.cols)) return PS_EINVAL;   // QU:67-69
    }
    QTensor& t = p.tensors[(size_t)i];
    t.fin = d.fvalue; t.fout = d.fvalue; t.codes = d.codes; t.diag = d.diagonal; t.bucket = d.bucket_size;
    t.colmax = nullptr; t.sarrive = nullptr;
    t.rows = d.rows; t.cols = d.cols; t.ld = d.ld; t.ldq = d.ldq;
    t.bits = d.bits; t.extract = d.extract_diagonal ? 1 : 0;
    t.vec4 = (d.cols % 4 == 0 && d.ld % 4 == 0 && d.ldq % 4 == 0 && quant_aligned(d.fvalue, 16) &&
              quant_aligned(d.codes, d.bits == 16 ? 8 : 4) && quant_aligned(d.bucket_size, 16)) ? 1 : 0;
    t.strips = (int)((d.cols + QW - 1) / QW);
    t.team = 1; t.small_w = 0; t.chunk0 = 0; t.chunks = 0;
    t.path = Q_EMPTY;
    p.total_cols += quant_pad4((size_t)d.cols);
    if (!nonempty) continue;
    const long long tiles = (long long)t.strips * ((d.rows + QR - 1) / QR);
    as_tiles += tiles;
    if (as_tiles > 0x7fffffffLL) return PS_EUNSUPPORTED;
    const bool flat_ok = t.vec4 && d.ld == d.cols && d.ldq == d.cols && quant_aligned(d.codes, 16) &&
                         d.cols <= QFLAT_MAXC && d.rows <= QMAXT / d.cols;   // rows * cols <= QMAXT
    long long* list = nullptr;
    long long n = 0;
    if (encode && flat_ok && d.rows >= QS_MINR && d.rows <= (long long)QS_MAX_TEAM * QS_ROWS) {
      t.path = Q_STRIP; list = &n_strip;
      t.team = (int)((d.rows + QS_ROWS - 1) / QS_ROWS);
      n = (d.cols + QS_COLS - 1) / QS_COLS * t.team;
      if (t.team > 1) p.team_strips += (size_t)(n / t.team);
    } else if (encode && d.rows <= QS_ROWS) {
      // short ones (rows < 64) of any width; others -- odd sizes, strided views -- up to 1024 rows
      t.path = Q_SMALL; list = &n_small;
      t.small_w = (int)std::min<long long>(std::min<long long>(d.cols, QSM_COLS), QSM_ELEMS / d.rows);
      n = (d.cols + t.small_w - 1) / t.small_w;
    } else if (flat_ok) {
      t.path = Q_FLAT; list = &n_flat;
      n = (d.rows * d.cols + QFLAT - 1) / QFLAT;
    } else {
      t.path = Q_TILE; list = &n_tile;
      n = tiles;
    }
    t.chunk0 = (int)*list;
    t.chunks = (int)n;
    *list += n;
    if (*list > 0x7fffffffLL) return PS_EUNSUPPORTED;
  }
  p.flat_chunks = (int)n_flat; p.tile_chunks = (int)n_tile; p.strip_items = (int)n_strip; p.small_items = (int)n_small;
  p.flat_off = 0;
  p.tile_off = p.flat_off + (size_t)n_flat;
  p.strip_off = p.tile_off + (size_t)n_tile;
  p.small_off = p.strip_off + (size_t)n_strip;
  p.table.resize(p.small_off + 2 * (size_t)n_small);
  const size_t off[5] = {0, p.strip_off, p.small_off, p.flat_off, p.tile_off};
  for (int i = 0; i < count; ++i) {
    const QTensor& t = p.tensors[(size_t)i];
    int* at = p.table.data() + off[t.path];
    if (t.path == Q_SMALL) {
      for (int k = 0; k < t.chunks; ++k) { at[2 * (t.chunk0 + k)] = i; at[2 * (t.chunk0 + k) + 1] = k * t.small_w; }
    } else if (t.path != Q_EMPTY) {
      std::fill_n(at + t.chunk0, (size_t)t.chunks, i);
    }
  }
  return PS_OK;
}

}  // namespace psk
