"""The C-ABI library loads on a GPU-less host and exports every symbol include/lvx.h declares; the product path refuses to
run without a HIP device (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def liblvx():
    import lvx
    if not os.path.exists(lvx.library_path()):
        subprocess.check_call(["python", os.path.join(ROOT, "lvi-exc_amd", "build.py")])
    return lvx.lib()


def _declared():
    src = open(os.path.join(ROOT, "include", "lvx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(lvx_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(liblvx):
    names = _declared()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(liblvx, n)]
    assert not missing, missing


LAYOUT_FIELDS = [("n_knots", 4), ("n_landmarks", 4), ("n_tangent", 4), ("n_band", 4), ("bandwidth", 4), ("n_border", 4), ("border_ld", 4), ("n_hub_knots", 4), ("hub_knot0", 4),
                 ("n_blocks", 8), ("n_residuals", 8), ("exact_fallback", 4), ("solver_fallbacks", 4), ("fallback_rows", 4), ("solver_separators", 4), ("solver_leaves", 4),
                 # appended for the landmark-track tests: which plan the last layout / the last solve took.  Fields are only ever added at the end.
                 ("rep_groups", 4), ("lm_groups", 4), ("lm_group_spread", 4), ("lm_row_width", 4), ("lm_elim_kernel", 4), ("rep_colours", 4)]


def test_layout_struct_matches_the_header():
    """lvx_layout of include/lvx.h, field by field, against the ctypes mirror lvx.Layout and the table above: names, order, widths, offsets (no earlier field moves when the struct
    grows) and the total size."""
    import lvx
    src = open(os.path.join(ROOT, "include", "lvx.h")).read()
    body = re.search(r"typedef struct lvx_layout \{(.*?)\} lvx_layout;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = []
    for typ, names in re.findall(r"\b(int32_t|int64_t)\s+([^;]+);", body):
        decl += [(n.strip(), 4 if typ == "int32_t" else 8) for n in names.split(",")]
    assert decl == LAYOUT_FIELDS
    assert [(n, C.sizeof(t)) for n, t in lvx.Layout._fields_] == LAYOUT_FIELDS
    off = 0
    for name, width in LAYOUT_FIELDS:
        off = (off + width - 1) // width * width
        assert getattr(lvx.Layout, name).offset == off, name
        off += width
    assert lvx.Layout.n_blocks.offset == 40 and lvx.Layout.solver_leaves.offset == 72 and lvx.Layout.rep_groups.offset == 76
    assert C.sizeof(lvx.Layout) == 104      # 100 bytes of fields, padded to the alignment of the int64 members


def test_no_device_means_error_not_fallback(liblvx):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import lvx
    h = C.c_void_p()
    assert liblvx.lvx_create(C.byref(h), 0, 0) == lvx.E_NODEVICE
    with pytest.raises(lvx.LvxError):
        lvx.Context(0)


def test_product_library_does_not_link_the_oracle(liblvx):
    import lvx
    out = subprocess.run(["ldd", lvx.library_path()], capture_output=True, text=True).stdout
    assert "oracle" not in out
    # and no vendor BLAS either: rocBLAS / rocSOLVER (bands wider than 208 only) and RCCL are dlopen'ed on demand — the library's link-time dependencies are the HIP runtime
    # and the C / C++ runtimes
    for lib in ("rocblas", "rocsolver", "hipblas", "rccl", "rocroller"):
        assert lib not in out, lib
    syms = subprocess.run(["nm", "-D", "--defined-only", lvx.library_path()], capture_output=True, text=True).stdout
    assert "orc_" not in syms


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("lvx_build_table", os.path.join(ROOT, "lvi-exc_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_source_names_its_fp_contract_mode():
    """build.py's CONTRACT table names every csrc/*.hip (no source falls through to a default) and names nothing that is gone.  Every file that holds upstream code
    (it includes lvx_stdsort.h or lvx_vxradius.h, which the host checks restate bit for bit) or is compared bit for bit against a g++ build of its header (render, traj,
    rotinit) is built without FMA contraction.  A source the table does not know is an error of the build, not a default."""
    mod = _build_module()
    csrc = os.path.join(ROOT, "lvi-exc_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert len(names) >= 9
    assert sorted(mod.CONTRACT) == names
    assert all(v in ("off", mod.DEFAULT) for v in mod.CONTRACT.values())
    upstream = [f for f in names if re.search(r'#include "lvx_(stdsort|vxradius)\.h"', open(os.path.join(csrc, f)).read())]
    assert "lvx_upstream.hip" in upstream
    for f in upstream + ["lvx_render.hip", "lvx_traj.hip", "lvx_rotinit.hip"]:
        assert mod.CONTRACT[f] == "off" and mod.contract(f) == "off", f
    assert mod.contract("lvx_eval") == mod.DEFAULT_CONTRACT and mod.contract(os.path.join(csrc, "lvx_upstream.hip")) == "off"
    with pytest.raises(RuntimeError):
        mod.contract("lvx_not_a_source.hip")
    # the experiment builds take the mode from the same table
    assert "build.py --contract" in open(os.path.join(ROOT, "tools", "build_variant.sh")).read()


def test_graft_entry_build():
    import importlib
    ge = importlib.import_module("__graft_entry__")
    so = ge.build()
    assert os.path.exists(so)
