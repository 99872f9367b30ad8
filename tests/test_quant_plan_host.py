"""CPU tests of the quantizer's host plan (precondition_amd/csrc/quant_plan.h): which path a tensor takes, the
per-chunk table the kernels index with blockIdx.x, and the bound the workspace queries reserve for it.
tests/quant_plan_host.cpp builds the SAME plan ps_quantize_f32 / ps_dequantize_f32 build; pointers in the
descriptors are made-up values with chosen alignment and are never dereferenced."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ps_quant_desc (include/ps_api.h)
DESC = np.dtype([("fvalue", "u8"), ("codes", "u8"), ("diagonal", "u8"), ("bucket_size", "u8"), ("rows", "i8"),
                 ("cols", "i8"), ("ld", "i8"), ("ldq", "i8"), ("bits", "i4"), ("extract_diagonal", "i4")], align=True)
EMPTY, STRIP, SMALL, FLAT, TILE = range(5)
PS_OK, PS_EINVAL, PS_EUNSUPPORTED = 0, -1, -3
BASE = 0x7000_0000_0000        # 256-byte aligned, like an allocation


def desc(rows, cols, bits=8, ld=None, ldq=None, extract=0, f_off=0, c_off=0, b_off=0, diag=True):
  d = np.zeros((), DESC)
  d["fvalue"], d["codes"], d["bucket_size"] = BASE + f_off, 2 * BASE + c_off, 3 * BASE + b_off
  d["diagonal"] = 4 * BASE if diag else 0
  d["rows"], d["cols"] = rows, cols
  d["ld"] = cols if ld is None else ld
  d["ldq"] = d["ld"] if ldq is None else ldq
  d["bits"], d["extract_diagonal"] = bits, extract
  return d


class Plan:
  def __init__(self, rc, tensors, totals, table):
    self.rc, self.tensors, self.table = rc, tensors, table
    (self.n_flat, self.n_tile, self.n_strip, self.n_small, self.flat_off, self.tile_off, self.strip_off,
     self.small_off, self.words, self.bound, self.total_cols, self.team_strips, self.scratch,
     self.scratch_bound) = (int(x) for x in totals)


@pytest.fixture(scope="module")
def build(tmp_path_factory):
  out = tmp_path_factory.mktemp("quant_plan") / "quant_plan_host.so"
  subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                         os.path.join(ROOT, "tests", "quant_plan_host.cpp"), "-o", str(out)])
  lib = ctypes.CDLL(str(out))
  lib.quant_plan_host.restype = ctypes.c_int

  def run(descs, encode, cap=1 << 18):
    tbl = np.array(descs, DESC)
    n = len(tbl)
    tensors = np.zeros((n, 6), np.int32)
    totals = np.zeros(14, np.int64)
    table = np.full(cap, -1, np.int32)
    rc = lib.quant_plan_host(ctypes.c_void_p(tbl.ctypes.data), ctypes.c_int(n), ctypes.c_int(int(encode)),
                             ctypes.c_void_p(tensors.ctypes.data), ctypes.c_void_p(totals.ctypes.data),
                             ctypes.c_void_p(table.ctypes.data), ctypes.c_longlong(cap))
    if rc == PS_OK:
      assert totals[8] <= cap
      table = table[:totals[8]]
    return Plan(rc, tensors, totals, table)
  return run


def one(build, d, encode):
  p = build([d], encode)
  assert p.rc == PS_OK
  path, vec4, team, small_w, chunk0, chunks = (int(x) for x in p.tensors[0])
  assert chunk0 == 0
  return dict(path=path, vec4=vec4, team=team, small_w=small_w, chunks=chunks)


@pytest.mark.parametrize("d,want", [
    (desc(1024, 1024), dict(path=STRIP, team=1, chunks=16)),
    (desc(3072, 768), dict(path=STRIP, team=3, chunks=36)),
    (desc(4096, 64), dict(path=STRIP, team=4)),
    (desc(4100, 64), dict(path=FLAT, chunks=17)),
    (desc(1000, 260), dict(path=STRIP, chunks=5)),
    (desc(63, 64), dict(path=SMALL)),
    (desc(200, 3), dict(path=SMALL, small_w=3, chunks=1)),
    (desc(1, 151296), dict(path=SMALL, small_w=2048, chunks=74)),
    (desc(1100, 7), dict(path=TILE, chunks=18)),
    (desc(1100, 260, ld=264), dict(path=TILE, vec4=1, chunks=36)),
    (desc(1030, 8196), dict(path=TILE, vec4=1, chunks=561)),
    (desc(512, 512, bits=16, c_off=8), dict(path=SMALL)),          # int16 codes aligned to 8 but not 16 bytes
    (desc(1 << 19, 4096), dict(path=TILE)),                        # more than 2^30 elements: 64-bit indices only
])
def test_quantize_classification(build, d, want):
  got = one(build, d, True)
  assert {k: got[k] for k in want} == want, got


@pytest.mark.parametrize("d,want", [
    (desc(1024, 1024), dict(path=FLAT, chunks=64)),
    (desc(200, 3), dict(path=TILE)),
    (desc(70, 260, bits=16, ld=264), dict(path=TILE, vec4=1)),
])
def test_dequantize_classification(build, d, want):
  got = one(build, d, False)
  assert {k: got[k] for k in want} == want, got


def refusal(descs):
  """The validation of a descriptor list, restated: the first offending tensor decides."""
  tiles = 0
  for d in descs:
    rows, cols = int(d["rows"]), int(d["cols"])
    if rows < 0 or cols < 0 or int(d["bits"]) not in (8, 16):
      return PS_EINVAL
    if rows > 0 and cols > 0:
      if not d["fvalue"] or not d["codes"] or not d["bucket_size"] or d["ld"] < cols or d["ldq"] < cols:
        return PS_EINVAL
      if d["extract_diagonal"] and (not d["diagonal"] or rows != cols):
        return PS_EINVAL
      tiles += -(-cols // 256) * -(-rows // 64)          # the call's size limit counts 64 x 256 tiles
    if tiles > 2 ** 31 - 1:
      return PS_EUNSUPPORTED
  return PS_OK


def check_invariants(build, descs, encode):
  p = build(descs, encode)
  assert p.rc == refusal(descs)
  if p.rc != PS_OK:
    return p
  assert (p.flat_off, p.tile_off, p.strip_off, p.small_off) == (
      0, p.n_flat, p.n_flat + p.n_tile, p.n_flat + p.n_tile + p.n_strip)
  assert p.words == p.n_flat + p.n_tile + p.n_strip + 2 * p.n_small == len(p.table)
  assert p.words <= p.bound
  assert p.scratch <= p.scratch_bound
  if not encode:
    assert p.n_strip == p.n_small == 0
  small = p.table[p.small_off:].reshape(-1, 2)
  lists = {FLAT: p.table[p.flat_off:p.tile_off], TILE: p.table[p.tile_off:p.strip_off],
           STRIP: p.table[p.strip_off:p.small_off], SMALL: small[:, 0]}
  path, team, small_w, chunk0, chunks = (p.tensors[:, k].astype(np.int64) for k in (0, 2, 3, 4, 5))
  nonempty = np.array([d["rows"] > 0 and d["cols"] > 0 for d in descs])
  assert ((path != EMPTY) == nonempty).all()
  assert (chunks[nonempty] > 0).all() and (chunks[~nonempty] == 0).all()
  for which, owners in lists.items():
    assert ((owners >= 0) & (owners < len(descs))).all()
    assert (path[owners] == which).all()                     # a tensor appears in the list of its path only ...
    idx = np.arange(len(owners))
    assert ((chunk0[owners] <= idx) & (idx < chunk0[owners] + chunks[owners])).all()
    assert len(owners) == chunks[path == which].sum()        # ... and with every one of its items
  cols = np.array([int(d["cols"]) for d in descs], np.int64)
  k = np.arange(len(small)) - chunk0[small[:, 0]]
  assert (small[:, 1] == k * small_w[small[:, 0]]).all() and (small[:, 1] < cols[small[:, 0]]).all()
  assert p.team_strips == sum(-(-cols[i] // 64) for i in range(len(descs)) if team[i] > 1)
  return p


def random_descs(rng):
  descs = []
  for _ in range(int(rng.integers(1, 9))):
    rows = int(rng.choice([0, 1, 3, 63, 64, 65, 100, 197, 1000, 1023, 1024, 1025, 2048, 3072, 4096, 4097, 5000]))
    cols = int(rng.choice([0, 1, 3, 4, 7, 64, 68, 260, 768, 1024, 2052, 8192, 8196, 20000]))
    if rng.uniform() < 0.3:
      cols = rows                                            # square: may extract
    pad = int(rng.choice([0, 0, 0, 4, 1]))
    d = desc(rows, cols, bits=int(rng.choice([8, 16])), ld=cols + pad,
             ldq=cols + (pad if rng.uniform() < 0.8 else 4),
             extract=int(rows == cols and rng.uniform() < 0.5),
             f_off=int(rng.choice([0, 0, 0, 4, 16])), c_off=int(rng.choice([0, 0, 0, 2, 4, 8, 16])),
             b_off=int(rng.choice([0, 0, 0, 4, 16])))
    bad = rng.uniform()
    if bad < 0.01:
      d["rows"] = -1
    elif bad < 0.02:
      d["bits"] = 4
    elif bad < 0.03:
      d["codes"] = 0
    elif bad < 0.04:
      d["ld"] = cols - 1
    elif bad < 0.05:
      d["extract_diagonal"] = 1                              # refused unless square with a diagonal buffer
      d["diagonal"] = 0 if rng.uniform() < 0.5 else d["diagonal"]
    descs.append(d)
  return descs


def test_invariants_over_random_descriptor_lists(build):
  rng = np.random.default_rng(2024)
  seen, refused = set(), 0
  for n in range(3000):
    descs = random_descs(rng)
    p = check_invariants(build, descs, encode=bool(n & 1))
    if p.rc == PS_OK:
      seen.update((n & 1, int(x)) for x in p.tensors[:, 0])
    else:
      refused += 1
  assert seen == {(1, EMPTY), (1, STRIP), (1, SMALL), (1, FLAT), (1, TILE), (0, EMPTY), (0, FLAT), (0, TILE)}
  assert 100 < refused < 1500


def test_invariants_over_the_vit_b_statistics(build):
  """The 395 statistics of tests/asan_host_driver.cpp (ViT-B/16), int16 and int8 alternating, diagonal extracted."""
  sizes = [768] * 284 + [1024] * 108 + [1000, 1000, 197]
  descs = [desc(n, n, bits=8 if i & 1 else 16, extract=1) for i, n in enumerate(sizes)]
  assert len(descs) == 395
  q = check_invariants(build, descs, True)
  assert q.n_flat == q.n_tile == 0 and q.n_small == 1 and q.n_strip == 284 * 12 + 110 * 16    # 197 x 197: small
  d = check_invariants(build, descs, False)
  assert d.n_tile == 4 and d.n_flat == sum(-(-n * n // 16384) for n in sizes[:-1])             # 197 x 197: 4 tiles


def test_size_limit_of_a_call(build):
  p = build([desc(1 << 31, 1 << 14)], True)          # 2^25 x 64 tiles of 64 x 256: past 2^31 - 1
  assert p.rc == PS_EUNSUPPORTED == refusal([desc(1 << 31, 1 << 14)])
