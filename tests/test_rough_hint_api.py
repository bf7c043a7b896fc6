"""CPU: the entry points of the rough motion search on the device are declared, exported, bound and wrapped; their structs
lie as the header says; the kernel is in both libraries without scratch memory; and every refusal returns SCHRO_HIP_EINVAL
with a message that names the chain and the level -- through schro_hip_rough_hint_check / schro_hip_rough_me_check, the
validation of the two batch calls without a context (no pointer is dereferenced, so made-up device addresses do)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import schroedinger_amd as sa
from schroedinger_amd import _lib
from test_analysis_api import kernel_notes, LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schro_hip.h")
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
CALLS = ("schro_hip_rough_hint_batch", "schro_hip_rough_me_batch", "schro_hip_rough_hint_check", "schro_hip_rough_me_check",
         "schro_rough_me_heirarchical_scan_hint_hip", "schro_rough_me_heirarchical_scan_hip")
STRUCTS = {"SchroHipRoughPlane": _lib.RoughPlane, "SchroHipRoughHintPicture": _lib.RoughHintPicture, "SchroHipRoughChain": _lib.RoughChain}


def header_members(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]|\[.*\]", "", n) for n in re.sub(r"^(const\s+)?\w+\s", "", decl).split(",")]
    return names


def test_header_declares_the_structs_and_the_calls():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int schro_hip_rough_hint_batch (SchroHipContext * ctx, const SchroHipRoughHintPicture * pictures, int npictures);",
                 "int schro_hip_rough_me_batch (SchroHipContext * ctx, const SchroHipRoughChain * chains, int nchains, int nohint_distance, "
                 "int hint_distance);",
                 "int schro_hip_rough_hint_check (const SchroHipRoughHintPicture * pictures, int npictures);",
                 "int schro_hip_rough_me_check (const SchroHipRoughChain * chains, int nchains, int nohint_distance, int hint_distance);",
                 "int schro_rough_me_heirarchical_scan_hint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame, const SchroHipParams * params, "
                 "int shift, int distance, int ref, const void *hint_motion_vectors, void *motion_vectors);",
                 "int schro_rough_me_heirarchical_scan_hip (SchroHipFrame * const *frames, SchroHipFrame * const *ref_frames, "
                 "const SchroHipParams * params, int n_levels, int ref, void *const *motion_fields);"):
        assert decl in flat, decl
    for name, cls in STRUCTS.items():
        assert header_members(text, name) == [f[0] for f in cls._fields_], name
    assert re.search(r"#define SCHRO_HIP_ROUGH_WAVES %d\b" % sa.ROUGH_WAVES, text)
    assert re.search(r"#define SCHRO_HIP_MAX_HIER_LEVELS %d\b" % sa.MAX_HIER_LEVELS, text) and sa.MAX_HIER_LEVELS == 8


def test_struct_layouts_match_the_header(tmp_path):
    lines = []
    for name, cls in STRUCTS.items():
        lines.append('  printf("%%zu", sizeof(%s));' % name)
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (name, f[0]) for f in cls._fields_]
        lines.append('  printf("\\n");')
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [list(map(int, line.split())) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    want = [[C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_] for cls in STRUCTS.values()]
    assert got == want


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in CALLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int
        assert hasattr(exp, name)
    for name in ("rough_hint_batch", "rough_me_batch", "rough_scan", "rough_scan_hint", "motion_field", "download_field"):
        assert callable(getattr(sa.Context, name, None)), name
    assert callable(sa.rough_hint_check) and callable(sa.rough_me_check)


def test_null_arguments_are_refused_with_a_message():
    lib = _lib.load()
    for call, args, word in ((lib.schro_hip_rough_hint_batch, (None, (_lib.RoughHintPicture * 1)(), 1), b"rough_hint_batch"),
                             (lib.schro_hip_rough_me_batch, (None, (_lib.RoughChain * 1)(), 1, 12, 4), b"rough_me_batch"),
                             (lib.schro_hip_rough_hint_check, (None, 1), b"rough_hint_batch"),
                             (lib.schro_hip_rough_me_check, (None, 1, 12, 4), b"rough_me_batch"),
                             (lib.schro_hip_rough_hint_check, ((_lib.RoughHintPicture * 1)(), 0), b"rough_hint_batch"),
                             (lib.schro_rough_me_heirarchical_scan_hint_hip, (None, None, None, 1, 4, 0, None, None), b"scan_hint_hip"),
                             (lib.schro_rough_me_heirarchical_scan_hip, (None, None, None, 2, 0, None), b"rough_me_heirarchical_scan_hip")):
        assert call(*args) == -1
        assert word in lib.schro_hip_last_error()


class Mem:
    """A made-up device address with the members the wrappers read."""

    def __init__(self, ptr, width=0, height=0, stride=0):
        self.ptr, self.width, self.height, self.stride = ptr, width, height, stride or width


PARAMS = dict(x_num_blocks=26, y_num_blocks=20, xbsep_luma=8, ybsep_luma=8)
FIELD_BYTES = 26 * 20 * 20


def hint_picture(**kw):
    """(frame, ref, extension, params, shift, distance, ref_index, hint, field) of a good picture, members replaced by kw."""
    base = 0x100000 * kw.pop("slot", 1)
    d = dict(frame=Mem(base, 100, 76, 128), ref=Mem(base + 0x10000, 100, 76, 128), ext=0, params=PARAMS, shift=1, dist=4, ref_index=0,
             hint=Mem(base + 0x20000), field=Mem(base + 0x30000))
    params = dict(d["params"], **{k: kw.pop(k) for k in list(kw) if k in PARAMS})
    d.update(kw, params=params)
    return tuple(d[k] for k in ("frame", "ref", "ext", "params", "shift", "dist", "ref_index", "hint", "field"))


def chain(n_levels=3, w=101, h=75, slot=1, **kw):
    base = 0x1000000 * slot
    levels = []
    for k in range(1, n_levels + 1):
        w, h = (w + 1) // 2, (h + 1) // 2
        levels.append((Mem(base + 0x20000 * k, w, h), Mem(base + 0x20000 * k + 0x10000, w, h), kw.get("ext", 0)))
    params = dict(x_num_blocks=13, y_num_blocks=10, xbsep_luma=8, ybsep_luma=8)
    params.update({k: kw[k] for k in kw if k in params})
    fields = [Mem(base + 0x400000 + 0x1000 * k) for k in range(n_levels)]
    return [levels, params, kw.get("ref_index", 0), fields]


def test_good_descriptions_pass():
    sa.rough_hint_check([hint_picture(), hint_picture(slot=2, shift=7, dist=20, ref_index=1, xbsep_luma=64, ybsep_luma=64)])
    sa.rough_me_check([chain(), chain(1, slot=2), chain(8, 4000, 3000, slot=3, ref_index=1)], 12, 4)
    sa.rough_me_check([chain()], 20, 1)
    # both references of one picture share its planes: inputs may overlap
    a, b = chain(), chain(slot=2, ref_index=1)
    b[0] = [(fa, rb, e) for (fa, _, e), (_, rb, _) in zip(a[0], b[0])]
    sa.rough_me_check([a, b])


HINT_REFUSALS = [
    (dict(x_num_blocks=0), "0 x 20 blocks"), (dict(y_num_blocks=0), "26 x 0 blocks"), (dict(x_num_blocks=-3), "blocks"),
    (dict(dist=0), "distance 0"), (dict(dist=-1), "distance -1"), (dict(dist=21), "window of 43"),
    (dict(xbsep_luma=65), "block of 65 x 8"), (dict(ybsep_luma=72), "block of 8 x 72"), (dict(xbsep_luma=0), "block of 0 x 8"),
    (dict(ref_index=2), "reference 2"), (dict(ref_index=-1), "reference -1"),
    (dict(shift=0), "shift of a hint level"), (dict(shift=8), "shift of a hint level"), (dict(shift=-1), "shift of a hint level"),
    (dict(frame=Mem(0x100000, 100, 76, 99)), "stride shorter than a row"),
    (dict(ref=Mem(0x110000, 100, 76, 64)), "stride shorter than a row"),
    (dict(hint=Mem(0x130000)), "overlaps"),                                     # the hint field is the output field
    (dict(hint=Mem(0x130000 + FIELD_BYTES - 20)), "overlaps"),                  # ... or shares its last record
    (dict(field=Mem(0x100000 + 128 * 75)), "overlaps"),                         # the field inside a plane
    (dict(field=Mem(0x130002)), "4-byte aligned"),
    (dict(field=Mem(0)), "NULL pointer"), (dict(hint=Mem(0)), "no hint field"), (dict(frame=Mem(0, 100, 76, 128)), "NULL pointer"),
    (dict(ext=-1), "extension -1"),
]


@pytest.mark.parametrize("change,word", HINT_REFUSALS, ids=[w.replace(" ", "_") + str(n) for n, (_, w) in enumerate(HINT_REFUSALS)])
def test_hint_level_refusals_name_the_picture_and_the_level(change, word):
    lib = _lib.load()
    pictures = [hint_picture(slot=2), hint_picture(**change)]
    arr = sa.rough_hint_pictures(pictures)
    assert lib.schro_hip_rough_hint_check(arr, 2) == -1          # SCHRO_HIP_EINVAL
    msg = lib.schro_hip_last_error().decode()
    assert msg.startswith("rough_hint_batch: picture 1") and word in msg, msg
    if "blocks" not in word and "block of" not in word and "reference" not in word:
        assert "level %d" % change.get("shift", 1) in msg, msg
    with pytest.raises(sa.SchroHipError):
        sa.rough_hint_check(pictures)
    # the batch call refuses the same before it looks at its context's device: no context, same answer or "bad arguments"
    assert lib.schro_hip_rough_hint_batch(None, arr, 2) == -1


def test_two_pictures_with_one_field_are_refused():
    a, b = hint_picture(slot=2), list(hint_picture())
    b[8] = a[8]
    with pytest.raises(sa.SchroHipError, match="overlaps the field of picture"):
        sa.rough_hint_check([a, tuple(b)])
    # a hint field that another picture of the call writes
    b = list(hint_picture())
    b[7] = a[8]
    with pytest.raises(sa.SchroHipError, match="overlaps"):
        sa.rough_hint_check([a, tuple(b)])


def test_chain_refusals_name_the_chain_and_the_level():
    def refused(chains, word, nohint=12, hint=4):
        with pytest.raises(sa.SchroHipError) as e:
            sa.rough_me_check(chains, nohint, hint)
        assert "rough_me_batch: chain %d" % (len(chains) - 1) in str(e.value) and word in str(e.value), str(e.value)
        return str(e.value)

    good = chain(slot=2)
    # (the distances are the call's: the first chain is named)
    assert "level 3" in refused([chain()], "distance 0", nohint=0)
    assert "level 3" in refused([chain()], "window of 43", nohint=21)
    assert "level 2" in refused([chain()], "distance -2", hint=-2)
    assert "level 2" in refused([chain()], "window of 51", hint=25)
    refused([good, chain(x_num_blocks=0)], "0 x 10 blocks")
    refused([good, chain(ybsep_luma=65)], "block of 8 x 65")
    refused([good, chain(ref_index=3)], "reference 3")
    refused([good, chain(0)], "0 levels")
    c = chain(8, 4000, 3000)
    c[0].append(c[0][-1])
    c[3].append(Mem(0x7000000))
    refused([good, c], "9 levels")
    # a plane that is not half of the level below it, rounded up
    c = chain()
    lv = c[0][1]
    c[0][1] = (Mem(lv[0].ptr, lv[0].width - 1, lv[0].height), Mem(lv[1].ptr, lv[1].width - 1, lv[1].height), 0)
    msg = refused([good, c], "half of level 1's 51x38 is 26x19")
    assert "level 2" in msg and "25x19" in msg
    c = chain()
    lv = c[0][2]
    c[0][2] = (Mem(lv[0].ptr, lv[0].width, lv[0].height + 1), Mem(lv[1].ptr, lv[1].width, lv[1].height + 1), 0)
    assert "level 3" in refused([good, c], "half of level 2's")
    # overlapping fields: inside a chain, between chains, a field over a plane
    c = chain()
    c[3][2] = Mem(c[3][1].ptr + 20)
    assert "level" in refused([good, c], "overlaps the field")
    c = chain()
    c[3][0] = good[3][1]
    refused([good, c], "overlaps the field of chain")
    c = chain()
    c[3][1] = Mem(c[0][0][1].ptr + 4)
    refused([good, c], "overlaps a plane")
    c = chain()
    c[0][0] = (Mem(c[0][0][0].ptr, 51, 38, 50), c[0][0][1], 0)
    assert "level 1" in refused([good, c], "stride shorter than a row")
    c = chain()
    c[3][1] = Mem(0)
    assert "level 2" in refused([good, c], "NULL pointer")


def test_the_new_sources_keep_to_the_allowed_preprocessor_guards_and_are_built():
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("rough_hint.hip", "plane_rough.cpp", "scan_common.h"):
        path = os.path.join(CSRC, name)
        assert os.path.exists(path), name
        bad = [line for line in open(path) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "rough_hint.hip" in srcs and "plane_rough.cpp" in srcs


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_the_kernel_is_built_without_scratch(lib, tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    mine = {n: v for n, v in notes.items() if "rough_hint_kernel" in n}
    assert len(mine) == 1, sorted(mine)
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] == 0, (n, v)       # (the LDS is sized by the launch)
        assert v["vgpr_count"] <= 128, (n, v)                   # 16 waves of one workgroup on four SIMDs


def test_committed_resource_usage_lists_the_kernel_without_scratch():
    text = open(os.path.join(ROOT, "profiles", "r16_rough_hint_resource_usage.txt")).read()
    rows = re.findall(r"^(rough_hint_kernel|metric_scan_kernel) VGPRs (\d+) SGPRs (\d+) LDS (\d+) scratch (\d+) spillV (\d+)", text, re.M)
    assert sorted(r[0] for r in rows) == ["metric_scan_kernel", "rough_hint_kernel"]
    assert all(int(r[4]) == 0 and int(r[5]) == 0 for r in rows)
