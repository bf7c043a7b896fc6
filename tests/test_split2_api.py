"""CPU: the entry points of the split-2 mode decision on the device are declared, exported, bound and wrapped; the struct
lies as the header says; both kernels are in both libraries without scratch memory; and every refusal returns
SCHRO_HIP_EINVAL with a message that names the picture -- through schro_hip_split2_check, the validation of
schro_hip_split2_batch without a context (no pointer is dereferenced, so made-up device addresses do)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import schroedinger_amd as sa
import split2_cases as K
from schroedinger_amd import _lib
from test_analysis_api import kernel_notes, LLVM
from test_rough_hint_api import header_members, Mem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
CALLS = ("schro_hip_split2_metric_batch", "schro_hip_split2_choose_batch", "schro_hip_split2_batch", "schro_hip_split2_check",
         "schro_mode_decision_split2_hip")


def test_header_declares_the_struct_and_the_calls():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int schro_hip_split2_metric_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n, void *const *tables);",
                 "int schro_hip_split2_choose_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n, void *const *tables);",
                 "int schro_hip_split2_batch (SchroHipContext * ctx, const SchroHipSplit2Picture * pictures, int n);",
                 "int schro_hip_split2_check (const SchroHipSplit2Picture * pictures, int n);",
                 "int schro_mode_decision_split2_hip (SchroHipFrame * src, SchroHipFrame * const *ref_upframes, const SchroHipParams * params, "
                 "double lambda, const void *const *subpel_fields, void *motion, void *superblocks);"):
        assert decl in flat, decl
    assert header_members(text, "SchroHipSplit2Picture") == [f[0] for f in _lib.Split2Picture._fields_]
    # the header derives the reach of the chroma reads, says what is out of scope, and pins the layout and the table entry
    assert "SCHRO_HIP_SIZE (SchroHipSplit2Picture, 184);" in text and "OUT OF SCOPE" in text
    assert "#define SCHRO_HIP_SPLIT2_TABLE_INTS %d" % sa.SPLIT2_TABLE_INTS in text
    assert text.count("REACH") >= 3


def test_struct_layout_matches_the_header(tmp_path):
    cls = _lib.Split2Picture
    lines = ['  printf("%zu", sizeof(SchroHipSplit2Picture));']
    lines += ['  printf(" %%zu", offsetof(SchroHipSplit2Picture, %s));' % f[0] for f in cls._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
    assert got[0] == 184
    assert sa.SB_DTYPE.itemsize == 16 and sa.SB_DTYPE.fields["score"][1] == 8


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in CALLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int
        assert hasattr(exp, name)
    for name in ("split2_metric_batch", "split2_choose_batch", "split2_batch", "mode_decision_split2"):
        assert callable(getattr(sa.Context, name, None)), name
    for name in ("split2_pictures", "split2_check"):
        assert callable(getattr(sa, name, None)), name


def test_null_arguments_are_refused_with_a_message():
    lib = _lib.load()
    one, tab = (_lib.Split2Picture * 1)(), (C.c_void_p * 1)()
    for call, args, word in ((lib.schro_hip_split2_metric_batch, (None, one, 1, tab), b"split2_metric_batch"),
                             (lib.schro_hip_split2_choose_batch, (None, one, 1, tab), b"split2_choose_batch"),
                             (lib.schro_hip_split2_batch, (None, one, 1), b"split2_batch"),
                             (lib.schro_hip_split2_check, (None, 1), b"split2_batch"),
                             (lib.schro_hip_split2_check, (one, 0), b"split2_batch"),
                             (lib.schro_mode_decision_split2_hip, (None, None, None, 0.1, None, None, None), b"mode_decision_split2_hip")):
        assert call(*args) == -1
        assert word in lib.schro_hip_last_error()


PARAMS = dict(x_num_blocks=16, y_num_blocks=12, xbsep_luma=8, ybsep_luma=8, mv_precision=2)
FIELD_BYTES = 16 * 12 * 20
KEYS = ("src", "refs", "shifts", "ext", "params", "lam", "fields", "motion", "superblocks")


def up_stride(w):
    return 512 * ((w + 79) // 16 + 1)


def picture(**kw):
    """(src, refs, shifts, extension, params, lambda, fields, motion, superblocks) of a good picture at made-up addresses,
    members replaced by kw."""
    base = 0x10000000 * kw.pop("slot", 1)
    w, h = kw.pop("w", 100), kw.pop("h", 76)
    hs, vs = shifts = kw.pop("shifts", (1, 1))
    nrefs = kw.pop("nrefs", 2)
    cw, ch = (w + hs) >> hs if hs in (0, 1) else w, (h + vs) >> vs if vs in (0, 1) else h
    stride = kw.pop("stride", 128)
    src = [Mem(base, w, h, stride), Mem(base + 0x100000, cw, ch, stride), Mem(base + 0x200000, cw, ch, stride)]
    refs = [[Mem(base + 0x1000000 * (r + 1) + 0x400000 * k, stride=up_stride(cw if k else w)) for k in range(3)] for r in range(nrefs)]
    d = dict(src=src, refs=refs, shifts=shifts, ext=32, params=PARAMS, lam=0.1,
             fields=[Mem(base + 0x8000000 + 0x10000 * r) for r in range(max(nrefs, 1))][:max(nrefs, 0) or 1], motion=Mem(base + 0x8100000),
             superblocks=Mem(base + 0x8200000))
    params = dict(d["params"], **{k: kw.pop(k) for k in list(kw) if k in PARAMS})
    d.update(kw, params=params)
    return tuple(d[k] for k in KEYS)


def replaced(p, **kw):
    d = dict(zip(KEYS, p))
    d.update(kw)
    return tuple(d[k] for k in KEYS)


def test_good_descriptions_pass():
    sa.split2_check([picture(), picture(slot=2, mv_precision=0, nrefs=1), picture(slot=3, mv_precision=3, xbsep_luma=32, ybsep_luma=32, lam=0),
                     picture(slot=4, ext=8, shifts=(0, 0)), picture(slot=5, xbsep_luma=4, ybsep_luma=4, ext=4, shifts=(1, 0), mv_precision=1)])
    # two pictures may share a reference, and a picture may be its own reference: inputs may overlap
    a, b = picture(), picture(slot=2)
    sa.split2_check([a, replaced(b, refs=a[1])])
    sa.split2_check([replaced(a, refs=[a[1][0], a[1][0]])])
    # both references may hand over the same field
    sa.split2_check([replaced(a, fields=[a[6][0], a[6][0]])])
    # the largest picture whose coordinates fit 16 bits at the precision
    sa.split2_check([picture(w=4091, h=100, mv_precision=3, stride=4096, x_num_blocks=512, y_num_blocks=16)])


GOOD = picture()
REFUSALS = [
    (dict(x_num_blocks=0), "0 x 12 blocks"), (dict(y_num_blocks=-4), "blocks"),
    (dict(x_num_blocks=13), "13 x 12 blocks are not whole superblocks"), (dict(y_num_blocks=10), "16 x 10 blocks are not whole superblocks"),
    (dict(mv_precision=4), "mv_precision 4 is outside 0 .. 3"), (dict(mv_precision=-1), "mv_precision -1"),
    (dict(xbsep_luma=36), "a block of 36 x 8 is outside 1 .. 32"), (dict(ybsep_luma=0), "a block of 8 x 0"),
    (dict(xbsep_luma=7), "a block of 7 x 8 is no multiple of the chroma subsampling"), (dict(ybsep_luma=5), "no multiple of the chroma subsampling"),
    (dict(nrefs=0), "0 references"), (dict(nrefs=3), "3 references"),
    (dict(shifts=(0, 1)), "chroma shifts 0,1 are none of"), (dict(shifts=(2, 1)), "chroma shifts 2,1"), (dict(shifts=(1, -1)), "chroma shifts 1,-1"),
    (dict(ext=7), "extension 7 is under the block separation 8"), (dict(ext=15, ybsep_luma=16), "extension 15 is under the block separation 16"),
    (dict(ext=33), "extension 33 is over the 32 apron columns"),
    (dict(w=4092, h=100, mv_precision=3, stride=4096), "a coordinate of 32768 does not fit"),
    (dict(stride=99), "component Y: stride 99 is shorter than a row of 100"), (dict(stride=49), "stride 49 is shorter"),
    (dict(lam=-0.5), "lambda -0.5 is negative or not finite"), (dict(lam=float("nan")), "negative or not finite"),
    (dict(lam=float("inf")), "negative or not finite"),
    (dict(src=[GOOD[0][0], None, GOOD[0][2]]), "component U of the picture is a NULL pointer"),
    (dict(src=[GOOD[0][0], GOOD[0][1], None]), "component V of the picture is a NULL pointer"),
    (dict(refs=[GOOD[1][0], [GOOD[1][1][0], GOOD[1][1][1], None]]), "the upsampled V image of reference 1 is a NULL pointer"),
    (dict(refs=[[None] + GOOD[1][0][1:], GOOD[1][1]]), "the upsampled Y image of reference 0 is a NULL pointer"),
    (dict(refs=[[Mem(GOOD[1][0][0].ptr + 64, stride=GOOD[1][0][0].stride)] + GOOD[1][0][1:], GOOD[1][1]]), "not 128-byte aligned"),
    # (one stride per component serves both references: the wrapper takes the last reference's)
    (dict(refs=[GOOD[1][0], [Mem(GOOD[1][1][0].ptr, stride=GOOD[1][1][0].stride - 512)] + GOOD[1][1][1:]]), "the upsampled Y image has a stride of"),
    (dict(fields=[GOOD[6][0], None]), "the field of reference 1 is a NULL pointer"),
    (dict(fields=[Mem(GOOD[6][0].ptr + 2), GOOD[6][1]]), "the field of reference 0 is not 4-byte aligned"),
    (dict(motion=None), "NULL pointer"), (dict(superblocks=None), "NULL pointer"),
    (dict(motion=Mem(GOOD[7].ptr + 2)), "aligned"), (dict(superblocks=Mem(GOOD[8].ptr + 4)), "aligned"),
    (dict(motion=Mem(GOOD[6][1].ptr + FIELD_BYTES - 20)), "the motion field overlaps a sub-pel field"),
    (dict(motion=Mem(GOOD[0][1].ptr + 128)), "the motion field overlaps the picture"),
    (dict(superblocks=Mem(GOOD[1][1][2].ptr + 4096)), "the superblock table overlaps an upsampled image"),
    (dict(superblocks=Mem(GOOD[7].ptr + 40)), "overlaps the motion field"),
]


@pytest.mark.parametrize("change,word", REFUSALS, ids=[re.sub(r"\W+", "_", w) + str(n) for n, (_, w) in enumerate(REFUSALS)])
def test_refusals_name_the_picture(change, word):
    lib = _lib.load()
    pictures = [picture(slot=2), picture(**change)]
    arr = sa.split2_pictures(pictures)
    assert lib.schro_hip_split2_check(arr, 2) == -1             # SCHRO_HIP_EINVAL
    msg = lib.schro_hip_last_error().decode()
    assert msg.startswith("split2_batch: picture 1") and word in msg, msg
    with pytest.raises(sa.SchroHipError):
        sa.split2_check(pictures)
    # the batch call refuses the same before it looks at its context's device: no context, same answer or "bad arguments"
    assert lib.schro_hip_split2_batch(None, arr, 2) == -1


def test_the_refusal_table_of_the_cases_is_covered_here():
    """Every member tests/split2_cases.py spoils on the device is refused on the host with the same words."""
    words = " ".join(w for _, w in REFUSALS)
    for member, value, word in K.REFUSED_MEMBERS:
        assert word.split()[0] in words, (member, word)


def test_outputs_of_two_pictures_must_not_overlap():
    a = picture(slot=2)
    with pytest.raises(sa.SchroHipError, match="picture 1: the motion field overlaps the motion field of picture 0"):
        sa.split2_check([a, picture(motion=a[7])])
    with pytest.raises(sa.SchroHipError, match="the superblock table overlaps the superblock table of picture"):
        sa.split2_check([a, picture(superblocks=a[8])])
    # a field that another picture of the call writes as its motion
    with pytest.raises(sa.SchroHipError, match="overlaps"):
        sa.split2_check([a, picture(fields=[a[7], picture()[6][1]])])
    # the single launches: the tables
    lib = _lib.load()
    arr = sa.split2_pictures([a, picture()])
    tabs = (C.c_void_p * 2)(0x7000000, 0x7100000)
    for call in (lib.schro_hip_split2_metric_batch, lib.schro_hip_split2_choose_batch):
        # (no context: refused as bad arguments before anything else; the table refusals need one and run on the device)
        assert call(None, arr, 2, tabs) == -1


def test_the_new_sources_keep_to_the_allowed_preprocessor_guards_and_are_built():
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("mode_split2.hip", "plane_split2.cpp"):
        path = os.path.join(CSRC, name)
        assert os.path.exists(path), name
        bad = [line for line in open(path) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "mode_split2.hip" in srcs and "plane_split2.cpp" in srcs
    text = open(os.path.join(CSRC, "mode_split2.hip")).read()
    # the score is not contracted into a fused multiply-add; the kernels hold no inline assembly
    assert "#pragma clang fp contract(off)" in text and "asm" not in re.sub(r"//.*", "", text)
    assert "__builtin_amdgcn_sad_u8" in text


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_the_kernels_are_built_without_scratch(lib, tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    mine = {n: v for n, v in notes.items() if "split2_metric_kernel" in n or "split2_choose_kernel" in n}
    assert len(mine) == 2, sorted(mine)
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["vgpr_count"] <= 128, (n, v)                   # four waves per SIMD at the least
        assert v["group_segment_fixed_size"] == 0, (n, v)       # neither kernel stages anything
