"""The int8-momentum transform descriptor: header, ctypes mirror and NumPy table dtype agree."""
import ctypes as C
import os
import re

from precondition_amd import _lib, kernels

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ps_api.h")


def _header_struct(name):
  """[(field, bytes)] of a header struct whose members are pointers and int64_t only."""
  src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
  body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
  fields = []
  for decl in (d.strip() for d in body.split(";")):
    if not decl:
      continue
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
    assert m, decl
    ctype, star, field = m.groups()
    assert star or ctype == "int64_t", decl
    fields.append((field, C.sizeof(C.c_void_p) if star else 8))
  return fields


def test_q8_descriptor_mirrors_have_the_header_structs_size():
  fields = _header_struct("ps_transform_q8_desc")
  size = sum(b for _, b in fields)   # 8-byte members only: no padding
  names = [f for f, _ in fields]
  assert names == [f for f, _ in _lib.TransformQ8Desc._fields_]
  assert names == list(kernels._TQDESC_DT.names)
  assert C.sizeof(_lib.TransformQ8Desc) == size == kernels._TQDESC_DT.itemsize
  for f in names:
    assert getattr(_lib.TransformQ8Desc, f).offset == kernels._TQDESC_DT.fields[f][1], f
  # the float32 descriptor is its prefix, unchanged
  assert names[:len(kernels._TDESC_DT.names)] == list(kernels._TDESC_DT.names)
  assert kernels._TDESC_DT.itemsize == C.sizeof(_lib.TransformDesc)
