"""CPU: the entry points of the sub-pel refinement on the device are declared, exported, bound and wrapped; the struct
lies as the header says; both kernels are in both libraries without scratch memory; and every refusal returns
SCHRO_HIP_EINVAL with a message that names the chain -- through schro_hip_subpel_check, the validation of
schro_hip_subpel_batch without a context (no pointer is dereferenced, so made-up device addresses do)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import schroedinger_amd as sa
from schroedinger_amd import _lib
from test_analysis_api import kernel_notes, LLVM
from test_rough_hint_api import header_members, Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
CALLS = ("schro_hip_subpel_error_batch", "schro_hip_subpel_choose_batch", "schro_hip_subpel_batch", "schro_hip_subpel_check",
         "schro_encoder_motion_predict_subpel_deep_hip")


def test_header_declares_the_struct_and_the_calls():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int schro_hip_subpel_error_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains, int mvprec, "
                 "void *const *tables);",
                 "int schro_hip_subpel_choose_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains, int mvprec, "
                 "void *const *tables);",
                 "int schro_hip_subpel_batch (SchroHipContext * ctx, const SchroHipSubpelChain * chains, int nchains);",
                 "int schro_hip_subpel_check (const SchroHipSubpelChain * chains, int nchains);",
                 "int schro_encoder_motion_predict_subpel_deep_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes, "
                 "const SchroHipParams * params, double lambda, void *const *subpel_fields);"):
        assert decl in flat, decl
    assert header_members(text, "SchroHipSubpelChain") == [f[0] for f in _lib.SubpelChain._fields_]
    # the header states the reach of the reads per precision, and pins the layout
    assert "REACH" in text and "SCHRO_HIP_SIZE (SchroHipSubpelChain, 88);" in text


def test_struct_layout_matches_the_header(tmp_path):
    cls = _lib.SubpelChain
    lines = ['  printf("%zu", sizeof(SchroHipSubpelChain));']
    lines += ['  printf(" %%zu", offsetof(SchroHipSubpelChain, %s));' % f[0] for f in cls._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
    assert got[0] == 88


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in CALLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int
        assert hasattr(exp, name)
    for name in ("subpel_error_batch", "subpel_choose_batch", "subpel_batch", "subpel_deep"):
        assert callable(getattr(sa.Context, name, None)), name
    for name in ("subpel_chains", "subpel_check"):
        assert callable(getattr(sa, name, None)), name


def test_null_arguments_are_refused_with_a_message():
    lib = _lib.load()
    one, tab = (_lib.SubpelChain * 1)(), (C.c_void_p * 1)()
    for call, args, word in ((lib.schro_hip_subpel_error_batch, (None, one, 1, 1, tab), b"subpel_error_batch"),
                             (lib.schro_hip_subpel_choose_batch, (None, one, 1, 1, tab), b"subpel_choose_batch"),
                             (lib.schro_hip_subpel_batch, (None, one, 1), b"subpel_batch"),
                             (lib.schro_hip_subpel_check, (None, 1), b"subpel_batch"),
                             (lib.schro_hip_subpel_check, (one, 0), b"subpel_batch"),
                             (lib.schro_encoder_motion_predict_subpel_deep_hip, (None, None, None, 0.1, None), b"subpel_deep_hip")):
        assert call(*args) == -1
        assert word in lib.schro_hip_last_error()


PARAMS = dict(x_num_blocks=13, y_num_blocks=10, xbsep_luma=8, ybsep_luma=8)
FIELD_BYTES = 13 * 10 * 20
KEYS = ("src", "up", "ext", "params", "prec", "ref_index", "lam", "src_field", "field")


def up_stride(w):
    return 512 * ((w + 79) // 16 + 1)


def chain(**kw):
    """(src, ref_up, extension, params, mv_precision, ref_index, lambda, src_field, field) of a good chain at made-up
    addresses, members replaced by kw."""
    base = 0x1000000 * kw.pop("slot", 1)
    w, h = kw.pop("w", 100), kw.pop("h", 76)
    d = dict(src=Mem(base, w, h, kw.pop("stride", 128)), up=Mem(base + 0x100000, stride=kw.pop("up_stride", up_stride(w))), ext=32, params=PARAMS,
             prec=2, ref_index=0, lam=0.1, src_field=Mem(base + 0x800000), field=Mem(base + 0x810000))
    params = dict(d["params"], **{k: kw.pop(k) for k in list(kw) if k in PARAMS})
    d.update(kw, params=params)
    return tuple(d[k] for k in KEYS)


def test_good_descriptions_pass():
    sa.subpel_check([chain(), chain(slot=2, prec=0), chain(slot=3, prec=3, ref_index=1, xbsep_luma=32, ybsep_luma=32, lam=0),
                     chain(slot=4, ext=8), chain(slot=5, xbsep_luma=4, ybsep_luma=4, ext=4, prec=1)])
    # in place: the source field is the destination
    f = Mem(0x1810000)
    sa.subpel_check([chain(src_field=f, field=f)])
    # both references of one picture share its plane; two pictures may share a reference: inputs may overlap
    a, b = chain(), chain(slot=2, ref_index=1)
    sa.subpel_check([a, (a[0],) + b[1:]])
    sa.subpel_check([a, (b[0], a[1]) + b[2:]])
    # the largest picture whose coordinates fit 16 bits at the precision
    sa.subpel_check([chain(w=4091, h=100, prec=3, stride=4096)])


REFUSALS = [
    (dict(x_num_blocks=0), "0 x 10 blocks"), (dict(y_num_blocks=0), "13 x 0 blocks"), (dict(y_num_blocks=-2), "blocks"),
    (dict(prec=4), "mv_precision 4 is outside 0 .. 3"), (dict(prec=-1), "mv_precision -1"),
    (dict(xbsep_luma=33), "a block of 33 x 8 is outside 1 .. 32"), (dict(ybsep_luma=36), "a block of 8 x 36"), (dict(xbsep_luma=0), "a block of 0 x 8"),
    (dict(ref_index=2), "reference 2"), (dict(ref_index=-1), "reference -1"),
    (dict(ext=7), "extension 7 is under the block separation 8"), (dict(ext=15, ybsep_luma=16), "extension 15 is under the block separation 16"),
    (dict(ext=33), "extension 33 is over the 32 apron columns"),
    (dict(w=4092, h=100, prec=3, stride=4096), "a coordinate of 32768 does not fit"), (dict(w=100, h=16368, prec=1), "a coordinate of 32768 does not fit"),
    (dict(stride=99), "stride 99 is shorter than a row of 100"),
    (dict(up=Mem(0x1100040, stride=up_stride(100))), "not 128-byte aligned"),
    (dict(up_stride=up_stride(100) - 512), "the upsampled image has a stride of"),
    (dict(lam=-0.5), "lambda -0.5 is negative or not finite"), (dict(lam=float("nan")), "negative or not finite"),
    (dict(lam=float("inf")), "negative or not finite"),
    (dict(src=Mem(0, 100, 76, 128)), "NULL pointer"), (dict(up=Mem(0, stride=up_stride(100))), "NULL pointer"), (dict(field=Mem(0)), "NULL pointer"),
    (dict(src_field=None), "NULL pointer"),
    (dict(field=Mem(0x1810002)), "4-byte aligned"),
    (dict(src_field=Mem(0x1810000 + 20)), "overlaps"),                          # the source field inside the field, not the field
    (dict(field=Mem(0x1000000 + 128 * 75)), "the field overlaps the picture"),
    (dict(field=Mem(0x1100000 + 4096)), "overlaps the upsampled image"),
]


@pytest.mark.parametrize("change,word", REFUSALS, ids=[re.sub(r"\W+", "_", w) + str(n) for n, (_, w) in enumerate(REFUSALS)])
def test_refusals_name_the_chain(change, word):
    lib = _lib.load()
    chains = [chain(slot=2), chain(**change)]
    arr = sa.subpel_chains(chains)
    assert lib.schro_hip_subpel_check(arr, 2) == -1             # SCHRO_HIP_EINVAL
    msg = lib.schro_hip_last_error().decode()
    assert msg.startswith("subpel_batch: chain 1") and word in msg, msg
    with pytest.raises(sa.SchroHipError):
        sa.subpel_check(chains)
    # the batch call refuses the same before it looks at its context's device: no context, same answer or "bad arguments"
    assert lib.schro_hip_subpel_batch(None, arr, 2) == -1


def test_fields_and_tables_of_two_chains_must_not_overlap():
    a = chain(slot=2)
    with pytest.raises(sa.SchroHipError, match="the field overlaps the field of chain"):
        sa.subpel_check([a, chain(field=a[8])])
    # a source field that another chain of the call writes
    with pytest.raises(sa.SchroHipError, match="overlaps"):
        sa.subpel_check([a, chain(src_field=a[8])])
    with pytest.raises(sa.SchroHipError, match="overlaps"):
        sa.subpel_check([a, chain(field=Mem(a[8].ptr + FIELD_BYTES - 20))])
    # the single-pass calls: the pass, and the tables
    lib = _lib.load()
    arr = sa.subpel_chains([a, chain()])
    tabs = (C.c_void_p * 2)(0x7000000, 0x7100000)
    for call in (lib.schro_hip_subpel_error_batch, lib.schro_hip_subpel_choose_batch):
        # (no context: refused as bad arguments before anything else; the refusals below need one and run on the device)
        assert call(None, arr, 2, 1, tabs) == -1


def test_the_new_sources_keep_to_the_allowed_preprocessor_guards_and_are_built():
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("subpel.hip", "plane_subpel.cpp"):
        path = os.path.join(CSRC, name)
        assert os.path.exists(path), name
        bad = [line for line in open(path) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "subpel.hip" in srcs and "plane_subpel.cpp" in srcs
    text = open(os.path.join(CSRC, "subpel.hip")).read()
    # the score is not contracted into a fused multiply-add; the kernels hold no inline assembly
    assert "#pragma clang fp contract(off)" in text and "asm" not in re.sub(r"//.*", "", text)
    assert "__builtin_amdgcn_sad_u8" in text


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_the_kernels_are_built_without_scratch(lib, tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    mine = {n: v for n, v in notes.items() if "subpel_error_kernel" in n or "subpel_choose_kernel" in n}
    assert len(mine) == 2, sorted(mine)
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["vgpr_count"] <= 128, (n, v)                   # four waves per SIMD at the least
        assert v["group_segment_fixed_size"] == (4096 if "error" in n else 0), (n, v)   # a 32 x 32 block per wave, four waves
