"""The geometry of every far operand tests/test_far_operands_gpu.py declares, by integer arithmetic on the CPU (nothing is allocated):
the pointer lies 4 GiB into the allocation, the allocation is within the 10 GiB cap, the last row starts 2^32 bytes or more behind the
pointer, every true offset and every 32-bit image of one (signed / unsigned, elements / bytes) lies inside the allocation, and an image
that differs from the true offset falls on the start of ANOTHER row of the operand or on a decoy the helper fills with other data --
never inside a row.  The planner gives the near and the far GEMM launch the same family.  The attention geometries would catch a K / V
tile offset held in 32 bits: the flash kernels' ``koff`` arithmetic restated in 32 and in 64 bits differs exactly where the entry
point's limit says so.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import gpu_checks as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometries():
    geos = []
    for fam, _bits, _glds, _naive in gc.FAR_GEMM_FAMILIES:
        for cname, words, fars in gc.far_gemm_specs(fam):
            for which in fars:
                r, c = gc.far_gemm_operand_rows(words, which)
                geos.append(gc.far_matrix_geometry(f"gemm[{fam}] {cname}: {which}", r, c, 2))
    geos += [gc.far_matrix_geometry(f"ff_fused {w}", 161, 320, 2) for w in ("X", "R", "Y")]
    for spec in gc.far_attention_specs():
        for which, via in spec["fars"]:
            geos.append(gc.far_attention_layout(spec, which, via)["geo"])
    geos += [gc.far_matrix_geometry(n, r, c, it) for n, r, c, it in gc.far_layout_geometries()]
    return geos


GEOS = _geometries()


@pytest.mark.parametrize("geo", GEOS, ids=[g["name"] for g in GEOS])
def test_far_geometry(geo):
    offs, cols, item, lead = geo["offsets"], geo["cols"], geo["item"], geo["lead"]
    assert lead >= 4 << 30 and lead % 16 == 0
    span = gc.far_span_bytes(geo)
    assert span <= gc.FAR_CAP
    assert len(np.unique(offs)) == len(offs) and offs.min() >= 0
    assert int(offs.max()) * item >= 1 << 32                          # the last row: 2^32 bytes or more behind the pointer
    if "ld" in geo:
        assert geo["ld"] & (geo["ld"] - 1) == 0 and geo["ld"] < 1 << 31    # a power of two that fits the ABI's int32
    lo, hi = -lead // item, (span - lead) // item                    # the allocation, in elements from the pointer
    assert lo <= offs.min() and offs.max() + cols <= hi
    rows = np.sort(offs)
    decoys = gc.far_decoys(geo)
    starts = np.sort(np.concatenate([rows, decoys]))
    assert (np.diff(starts) >= cols).all()                            # rows and decoys never overlap
    moved = 0
    for kind, img in gc.far_images(geo).items():
        assert (img >= lo).all() and (img + cols <= hi).all(), kind  # inside the allocation
        assert (img <= offs).all() and ((offs - img) * item <= 1 << 33).all(), kind   # between the pointer - 4 GiB and the true offset
        differs = img != offs
        moved += int(differs.sum())
        on_row = np.isin(img[differs], rows)
        on_decoy = np.isin(img[differs], decoys)
        assert (on_row | on_decoy).all(), kind                       # ... and on the start of another row, or on a decoy
    assert moved > 0                                                  # some image of some row differs: the case can fail


def test_power_of_two_images_fall_on_rows_of_the_operand():
    """With a power-of-two stride the unsigned byte image of row r (at or past 2^32 bytes) is the start of row r - 2^32 / (stride bytes):
    the example of the far-K case, 2^26 elements per key, sends key r >= 32 to key r - 32."""
    spec = next(s for s in gc.far_attention_specs() if s["Sk"] == 40 and s["kernel"] == "4-wave flash")
    L = gc.far_attention_layout(spec, "K", "seq")
    assert gc.FAR_ATTN_SEQ_ROWS * L["ld"] == 1 << 26
    offs = L["geo"]["offsets"].reshape(spec["batch"], spec["Sk"])
    img = gc.far_images(L["geo"])["unsigned bytes"].reshape(spec["batch"], spec["Sk"])
    assert (img[:, 32:] == offs[:, :8]).all() and (img[:, :32] == offs[:, :32]).all()


def _koff(row, dpc, kv_seq, ld, bits):
    """The K source offset of attention.hip (flash_attn_d64_v2_kernel, ``koff[t]``): bytes of key row ``row`` of a tile, chunk ``dpc``."""
    v = (row * kv_seq * ld + ((dpc ^ ((row >> 1) & 7)) << 3)) * 2
    return v & 0xFFFFFFFF if bits == 32 else v


FLASH = ("4-wave flash", "8-wave", "shared-softmax 4-wave", "shared-softmax 8-wave")
KV_CASES = [(s, w, v) for s in gc.far_attention_specs() if s["kernel"] in FLASH for w, v in s["fars"] if w in ("K", "V")]


@pytest.mark.parametrize("spec,which,via", KV_CASES, ids=[f"{s['name']}: {w} via {v}" for s, w, v in KV_CASES])
def test_flash_tile_offsets_in_32_bits_differ_exactly_beyond_the_limit(spec, which, via):
    L = gc.far_attention_layout(spec, which, via)
    kv_seq, ld = L["strides"][2], L["ld"]
    keys = min(64, spec["Sk"])
    wraps = [r for r in range(keys) for c in range(8) if _koff(r, c, kv_seq, ld, 32) != _koff(r, c, kv_seq, ld, 64)]
    assert bool(wraps) == L["fallback"] == (not gc.flash_tile_offsets_fit(kv_seq, ld, spec["heads"] * 64))
    if via.startswith("limit"):
        assert L["fallback"] == via.endswith("+8") and (not wraps or min(wraps) == 63)   # only key 63 is past 2^32 bytes
    if via == "seq" and spec["Sk"] == 40:
        assert wraps and min(wraps) == 32          # 2^26 elements per key: keys 32 .. 39 would be read as keys 0 .. 7


def test_some_flash_case_of_each_block_form_takes_the_fallback():
    took = {s["kernel"] for s, w, v in KV_CASES if gc.far_attention_layout(s, w, v)["fallback"]}
    assert {"4-wave flash", "shared-softmax 4-wave"} <= took


def test_limit_of_the_entry_point():
    assert gc.flash_tile_offsets_fit(4096, 960, 960)                       # temporal attention at 64 x 64, the widest level
    assert gc.FLASH_LIMIT_LD == 34087040
    assert gc.flash_tile_offsets_fit(1, 34087041, 8) and not gc.flash_tile_offsets_fit(1, 34087042, 8)
    assert not gc.flash_tile_offsets_fit(-1, 64, 64)


def test_planner_gives_near_and_far_gemm_launches_the_same_family(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "gemm_plan_main.cpp"),
                    os.path.join(ROOT, "anyv2v_amd", "csrc", "gemm_plan.cpp"), "-o", exe], check=True)
    rows = gc.far_gemm_plan_rows()
    out = subprocess.run([exe], input="".join(d + "\n" for _n, d in rows), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    plans = {n: json.loads(line) for (n, _d), line in zip(rows, out.stdout.splitlines())}
    assert len(plans) == len(rows)
    want = {"128-row reg": "mfma128", "128-row glds": "mfma128", "naive": "naive", "persistent 192x320": "big", "ping-pong 192": "pp", "ping-pong 256": "pp",
            "one-wave-per-SIMD": "sw", "stream-K": "sw_streamk", "LDS patch": "swh", "weight-stationary": "ws", "weight-stationary + LayerNorm": "ws_ln",
            "split-K": "mfma128"}
    near = None
    for name, plan in plans.items():
        assert plan["status"] == 0, (name, plan)
        fam = name.split(" | ")[0]
        assert plan["family"] == want[fam], (name, plan)
        if name.endswith("| near"):
            near = plan
        else:
            keys = ("family", "nf", "splits", "tilesN", "tiles", "grid", "pp_mf", "sk_blocks")
            assert [plan.get(k) for k in keys] == [near.get(k) for k in keys], (name, plan, near)
        if fam == "split-K":
            assert plan["splits"] > 1


def _lib_or_skip():
    from anyv2v_amd import _lib
    try:
        return _lib, _lib.load()
    except OSError as e:      # the library is built by __graft_entry__.build()
        pytest.skip(f"libanyv2v_hip.so not loadable: {e}")


def test_convolution_whose_source_rows_do_not_fit_an_int_is_rejected_before_any_launch():
    """Stride 2 from 2 x 2 to 1 x 1: 2^30 output rows read 2^32 source rows, which the kernels' int row numbers cannot hold."""
    import ctypes as C
    _lib, lib = _lib_or_skip()
    d = _lib.GemmDesc()
    d.A0, d.W, d.C = 1 << 20, 2 << 20, 3 << 20           # never dereferenced: the check returns first
    d.M, d.N, d.C0, d.lda0, d.ldc = 1 << 30, 320, 64, 64, 320
    d.mode, d.Hi, d.Wi, d.Ho, d.Wo, d.stride = 1, 2, 2, 1, 1, 2
    d.flags = _lib.ANYV2V_GEMM_LDS_DMA
    assert lib.anyv2v_gemm_f16(C.byref(d), None) == -1
    assert b"source has 2^31 rows or more" in lib.anyv2v_last_error()


def test_cfg_ddim_step_whose_pixel_count_does_not_fit_an_int_is_rejected_before_any_launch():
    _lib, lib = _lib_or_skip()
    rc = lib.anyv2v_cfg_ddim_step_f16(1 << 20, 8, 0, 1, 7.5, 2 << 20, 3 << 20, 4 << 20, 4, 65536, 65536, None)
    assert rc == -1 and b"F * HW must fit an int" in lib.anyv2v_last_error()


def test_attention_with_a_negative_leading_dimension_is_rejected():
    import ctypes as C
    _lib, lib = _lib_or_skip()
    d = _lib.AttnDesc()
    d.Q, d.K, d.V, d.O = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    d.ldq, d.ldk, d.ldv, d.ldo = 64, -64, 64, 64
    d.batch, d.heads, d.Sq, d.Sk, d.inner, d.kv_div = 1, 1, 40, 40, 1, 1
    d.q_outer, d.q_seq, d.kv_outer, d.kv_seq, d.scale = 40, 1, 40, 1, 0.125
    assert lib.anyv2v_attention_f16(C.byref(d), None) == -1
    assert b"leading dimensions must be positive" in lib.anyv2v_last_error()
