// quant_plan_host.cpp — CPU driver of precondition_amd/csrc/quant_plan.h (test infrastructure only).
//
// Builds the host plan of ps_quantize_f32 / ps_dequantize_f32 for a descriptor list and hands its contents to
// tests/test_quant_plan_host.py, which compiles this file with g++.  Pointers in the descriptors are never
// dereferenced.
#include <string.h>

#include "../precondition_amd/csrc/quant_plan.h"

using namespace psk;

enum { QP_TENSOR_FIELDS = 6, QP_TOTALS = 14 };

// tensors[count][6]: path, vec4, team, small_w, chunk0, chunks
// totals[14]: list lengths (flat, tile, strip, small), list offsets (same order), table words, table bound, total_cols,
//             team_strips, scratch words, scratch bound
// table[table_cap]: the per-chunk table, as far as it fits.  Returns the builder's code.
extern "C" int quant_plan_host(const ps_quant_desc* desc, int count, int encode, int* tensors, long long* totals,
                               int* table, long long table_cap) {
  QuantPlan p;
  const int rc = quant_build_plan(desc, count, encode != 0, p);
  if (rc != PS_OK) return rc;
  for (int i = 0; i < count; ++i) {
    const QTensor& t = p.tensors[(size_t)i];
    const int row[QP_TENSOR_FIELDS] = {t.path, t.vec4, t.team, t.small_w, t.chunk0, t.chunks};
    memcpy(tensors + (size_t)i * QP_TENSOR_FIELDS, row, sizeof(row));
  }
  const long long tot[QP_TOTALS] = {p.flat_chunks, p.tile_chunks, p.strip_items, p.small_items,
                                    (long long)p.flat_off, (long long)p.tile_off, (long long)p.strip_off,
                                    (long long)p.small_off, (long long)p.table.size(),
                                    (long long)quant_table_bound(desc, count), (long long)p.total_cols,
                                    (long long)p.team_strips, (long long)p.scratch_words(),
                                    (long long)quant_scratch_bound(desc, count)};
  memcpy(totals, tot, sizeof(tot));
  const size_t n = p.table.size() < (size_t)table_cap ? p.table.size() : (size_t)table_cap;
  if (n) memcpy(table, p.table.data(), n * sizeof(int));
  return PS_OK;
}
