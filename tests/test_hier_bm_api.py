"""CPU: the entry points of the hierarchical block matching on the device are declared, exported, bound and wrapped; their
structs lie as the header says; the kernel is in both libraries without scratch memory; and every refusal returns
SCHRO_HIP_EINVAL with a message that names the entry (or chain) and the level -- through schro_hip_hbm_level_check /
schro_hip_hbm_check, the validation of the two batch calls without a context (no pointer is dereferenced, so made-up
device addresses do)."""
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
CALLS = ("schro_hip_hbm_level_batch", "schro_hip_hbm_batch", "schro_hip_hbm_level_check", "schro_hip_hbm_check",
         "schro_hierarchical_bm_scan_hint_hip", "schro_hbm_scan_hip")


def structs():
    return {"SchroHipHbmPlane": _lib.HbmPlane, "SchroHipHbmLevel": _lib.HbmLevel, "SchroHipHbmChain": _lib.HbmChain}


def test_header_declares_the_structs_and_the_calls():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    for decl in ("int schro_hip_hbm_level_batch (SchroHipContext * ctx, const SchroHipHbmLevel * levels, int nlevels);",
                 "int schro_hip_hbm_batch (SchroHipContext * ctx, const SchroHipHbmChain * chains, int nchains, int with_level0);",
                 "int schro_hip_hbm_level_check (const SchroHipHbmLevel * levels, int nlevels);",
                 "int schro_hip_hbm_check (const SchroHipHbmChain * chains, int nchains, int with_level0);",
                 "int schro_hierarchical_bm_scan_hint_hip (SchroHipFrame * frame, SchroHipFrame * ref_frame, const SchroHipParams * params, "
                 "int shift, int h_range, int ref, const void *hint_motion_vectors, void *motion_vectors);",
                 "int schro_hbm_scan_hip (SchroHipFrame * const *frames, SchroHipFrame * const *ref_frames, const SchroHipParams * params, "
                 "int n_levels, int ref, int with_level0, void *const *motion_fields);"):
        assert decl in flat, decl
    for name, cls in structs().items():
        assert header_members(text, name) == [f[0] for f in cls._fields_], name
    # what the header must say about the chroma scan it does not cover
    assert "enable_chroma_me" in text and "schrometric.c:84-111" in text


def test_struct_layouts_match_the_header(tmp_path):
    lines = []
    for name, cls in structs().items():
        lines.append('  printf("%%zu", sizeof(%s));' % name)
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (name, f[0]) for f in cls._fields_]
        lines.append('  printf("\\n");')
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "schro_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [list(map(int, line.split())) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    want = [[C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_] for cls in structs().values()]
    assert got == want


def test_library_exports_and_binds_them():
    lib = _lib.load()
    exp = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libschro_hip_exp.so"))
    for name in CALLS:
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype == C.c_int
        assert hasattr(exp, name)
    for name in ("hbm_level_batch", "hbm_batch", "hbm_scan_hint", "hbm_scan"):
        assert callable(getattr(sa.Context, name, None)), name
    for name in ("hbm_levels", "hbm_chains", "hbm_level_check", "hbm_check"):
        assert callable(getattr(sa, name, None)), name


def test_null_arguments_are_refused_with_a_message():
    lib = _lib.load()
    for call, args, word in ((lib.schro_hip_hbm_level_batch, (None, (_lib.HbmLevel * 1)(), 1), b"hbm_level_batch"),
                             (lib.schro_hip_hbm_batch, (None, (_lib.HbmChain * 1)(), 1, 1), b"hbm_batch"),
                             (lib.schro_hip_hbm_level_check, (None, 1), b"hbm_level_batch"),
                             (lib.schro_hip_hbm_check, (None, 1, 0), b"hbm_batch"),
                             (lib.schro_hip_hbm_level_check, ((_lib.HbmLevel * 1)(), 0), b"hbm_level_batch"),
                             (lib.schro_hierarchical_bm_scan_hint_hip, (None, None, None, 1, 4, 0, None, None), b"bm_scan_hint_hip"),
                             (lib.schro_hbm_scan_hip, (None, None, None, 2, 0, 1, None), b"hbm_scan_hip")):
        assert call(*args) == -1
        assert word in lib.schro_hip_last_error()


PARAMS = dict(x_num_blocks=26, y_num_blocks=20, xbsep_luma=8, ybsep_luma=8)
FIELD_BYTES = 26 * 20 * 20
KEYS = ("frame", "ref", "ext", "h_shift", "v_shift", "params", "shift", "h_range", "ref_index", "hint", "field")


def planes(base, w, h, hs=1, vs=1, stride=None):
    """(Y, U, V) at made-up addresses 0x4000 apart."""
    cw, ch = (w + (1 << hs) - 1) >> hs, (h + (1 << vs) - 1) >> vs
    return (Mem(base, w, h, stride or 128), Mem(base + 0x4000, cw, ch, 64 if hs else 128), Mem(base + 0x8000, cw, ch, 64 if hs else 128))


def level(**kw):
    """(frame, ref, extension, h_shift, v_shift, params, shift, h_range, ref_index, hint, field) of a good entry, members replaced by kw."""
    base = 0x100000 * kw.pop("slot", 1)
    hs, vs = kw.get("h_shift", 1), kw.get("v_shift", 1)
    good = hs in (0, 1) and vs in (0, 1)
    d = dict(frame=planes(base, 100, 76, hs if good else 1, vs if good else 1), ref=planes(base + 0x10000, 100, 76, hs if good else 1, vs if good else 1),
             ext=32, h_shift=1, v_shift=1, params=PARAMS, shift=1, h_range=5, ref_index=0, hint=Mem(base + 0x20000), field=Mem(base + 0x30000))
    params = dict(d["params"], **{k: kw.pop(k) for k in list(kw) if k in PARAMS})
    d.update(kw, params=params)
    return tuple(d[k] for k in KEYS)


def chain(n_levels=3, w=101, h=75, slot=1, **kw):
    """[levels, h_shift, v_shift, params, ref_index, fields] with levels 0 .. n_levels."""
    base = 0x1000000 * slot
    levels = []
    for k in range(n_levels + 1):
        levels.append((planes(base + 0x20000 * k, w, h, stride=max(128, w)), planes(base + 0x20000 * k + 0x10000, w, h, stride=max(128, w)),
                       kw.get("ext", 32)))
        w, h = (w + 1) // 2, (h + 1) // 2
    params = dict(x_num_blocks=16, y_num_blocks=12, xbsep_luma=8, ybsep_luma=8)
    params.update({k: kw[k] for k in kw if k in params})
    fields = [Mem(base + 0x400000 + 0x1000 * k) for k in range(n_levels + 1)]
    return [levels, kw.get("h_shift", 1), kw.get("v_shift", 1), params, kw.get("ref_index", 0), fields]


def test_good_descriptions_pass():
    sa.hbm_level_check([level(), level(slot=2, shift=8, h_range=20, ref_index=1, xbsep_luma=64, ybsep_luma=64, ext=64),
                        level(slot=3, shift=0, hint=None), level(slot=4, h_shift=0, v_shift=0), level(slot=5, h_shift=1, v_shift=0)])
    sa.hbm_check([chain(), chain(1, slot=2), chain(8, 128, 100, slot=3, ref_index=1)], True)
    sa.hbm_check([chain()], False)
    # without level 0 its planes and its field are not read
    c = chain()
    c[0][0], c[5][0] = None, None
    sa.hbm_check([c], False)
    # both references of one picture share its planes: inputs may overlap
    a, b = chain(), chain(slot=2, ref_index=1)
    b[0] = [(fa, rb, e) for (fa, _, e), (_, rb, _) in zip(a[0], b[0])]
    sa.hbm_check([a, b])


def with_plane(which, k, **kw):
    """The planes of a good entry with component k of `which` replaced."""
    t = list(level()[KEYS.index(which)])
    m = t[k]
    t[k] = Mem(kw.get("ptr", m.ptr), m.width, m.height, kw.get("stride", m.stride))
    return {which: tuple(t)}


LEVEL_REFUSALS = [
    (dict(x_num_blocks=0), "0 x 20 blocks"), (dict(y_num_blocks=0), "26 x 0 blocks"), (dict(x_num_blocks=-3), "blocks"),
    (dict(h_range=0), "h_range 0"), (dict(h_range=-1), "h_range -1"), (dict(h_range=21), "window of 43"),
    (dict(xbsep_luma=65), "block of 65 x 8"), (dict(ybsep_luma=72), "block of 8 x 72"), (dict(xbsep_luma=0), "block of 0 x 8"),
    (dict(ref_index=2), "reference 2"), (dict(ref_index=-1), "reference -1"),
    (dict(shift=9), "shift of a level"), (dict(shift=-1), "shift of a level"),
    (dict(h_shift=2), "chroma shifts 2, 1"), (dict(h_shift=0, v_shift=1), "chroma shifts 0, 1"), (dict(v_shift=-1), "chroma shifts 1, -1"),
    (with_plane("frame", 0, stride=99), "component 0 has a stride shorter than a row of 100"),
    (with_plane("ref", 2, stride=49), "component 2 has a stride shorter than a row of 50"),
    (with_plane("frame", 1, ptr=0), "component 1 has a NULL pointer"), (with_plane("ref", 0, ptr=0), "component 0 has a NULL pointer"),
    (with_plane("ref", 2, ptr=0), "component 2 has a NULL pointer"),
    (dict(hint=Mem(0x130000)), "overlaps"),                                     # the hint field is the output field
    (dict(hint=Mem(0x130000 + FIELD_BYTES - 20)), "overlaps"),                  # ... or shares its last record
    (dict(field=Mem(0x100000 + 128 * 75)), "overlaps"),                         # the field inside the luma plane
    (dict(field=Mem(0x108000 + 64 * 37)), "overlaps"),                          # ... inside a chroma plane
    (dict(field=Mem(0x130002)), "4-byte aligned"), (dict(field=Mem(0)), "the field is a NULL pointer"),
    (dict(ext=-1), "extension -1"), (dict(ext=7), "extension 7 is under the block separation 8"),
    (dict(ext=15, ybsep_luma=16), "extension 15 is under the block separation 16"), (dict(ext=2000), "extension 2000"),
]


@pytest.mark.parametrize("change,word", LEVEL_REFUSALS, ids=[w.replace(" ", "_") + str(n) for n, (_, w) in enumerate(LEVEL_REFUSALS)])
def test_level_refusals_name_the_entry_and_the_level(change, word):
    lib = _lib.load()
    levels = [level(slot=2), level(**change)]
    arr = sa.hbm_levels(levels)
    assert lib.schro_hip_hbm_level_check(arr, 2) == -1          # SCHRO_HIP_EINVAL
    msg = lib.schro_hip_last_error().decode()
    assert msg.startswith("hbm_level_batch: entry 1") and word in msg, msg
    if "blocks" not in word and "block of" not in word and "reference" not in word:
        assert "level %d" % change.get("shift", 1) in msg, msg
    with pytest.raises(sa.SchroHipError):
        sa.hbm_level_check(levels)
    # the batch call refuses the same before it looks at its context's device: no context, same answer or "bad arguments"
    assert lib.schro_hip_hbm_level_batch(None, arr, 2) == -1


def test_two_entries_with_one_field_are_refused():
    a, b = level(slot=2), list(level())
    b[10] = a[10]
    with pytest.raises(sa.SchroHipError, match="overlaps the field of entry"):
        sa.hbm_level_check([a, tuple(b)])
    # a hint field that another entry of the call writes
    b = list(level())
    b[9] = a[10]
    with pytest.raises(sa.SchroHipError, match="overlaps"):
        sa.hbm_level_check([a, tuple(b)])


def test_chain_refusals_name_the_chain_and_the_level():
    def refused(chains, word, with_level0=True):
        with pytest.raises(sa.SchroHipError) as e:
            sa.hbm_check(chains, with_level0)
        assert "hbm_batch: chain %d" % (len(chains) - 1) in str(e.value) and word in str(e.value), str(e.value)
        return str(e.value)

    good = chain(slot=2)
    refused([good, chain(x_num_blocks=0)], "0 x 12 blocks")
    refused([good, chain(ybsep_luma=65)], "block of 8 x 65")
    refused([good, chain(ref_index=3)], "reference 3")
    refused([good, chain(0)], "0 levels")
    c = chain(8, 128, 100)
    c[0].append(c[0][-1])
    c[5].append(Mem(0x7000000))
    refused([good, c], "9 levels")
    assert "level 3" in refused([good, chain(ext=7)], "extension 7 is under the block separation 8")
    assert "level 3" in refused([good, chain(h_shift=1, v_shift=2)], "chroma shifts 1, 2")
    # a plane that is not half of the level below it, rounded up
    c = chain()
    f, r, e = c[0][2]
    c[0][2] = (planes(f[0].ptr, 25, 19), planes(r[0].ptr, 25, 19), e)
    msg = refused([good, c], "half of level 1's 51x38 is 26x19")
    assert "level 2" in msg and "25x19" in msg
    c = chain(1)
    f, r, e = c[0][1]
    c[0][1] = (planes(f[0].ptr, 51, 39), planes(r[0].ptr, 51, 39), e)
    assert "level 1" in refused([good, c], "half of level 0's 101x75 is 51x38")
    sa.hbm_check([good, c], False)             # (level 0 only takes part when it runs)
    # overlapping fields: inside a chain, between chains, a field over a plane
    c = chain()
    c[5][2] = Mem(c[5][1].ptr + 20)
    assert "level" in refused([good, c], "overlaps the field")
    c = chain()
    c[5][0] = good[5][1]
    refused([good, c], "overlaps the field of chain")
    sa.hbm_check([good, c], False)             # (field 0 is not read without level 0)
    c = chain()
    c[5][1] = Mem(c[0][1][1][2].ptr + 4)
    refused([good, c], "overlaps a plane")
    c = chain()
    f, r, e = c[0][1]
    c[0][1] = ((Mem(f[0].ptr, 51, 38, 50), f[1], f[2]), r, e)
    assert "level 1" in refused([good, c], "stride shorter than a row")
    c = chain()
    c[5][2] = Mem(0)
    assert "level 2" in refused([good, c], "NULL pointer")
    c = chain()
    c[5][0] = Mem(0)
    assert "level 0" in refused([good, c], "NULL pointer")


def test_the_new_sources_keep_to_the_allowed_preprocessor_guards_and_are_built():
    allowed = re.compile(r"^\s*#\s*(ifdef|ifndef|if)\s+(defined\s*\(?\s*)?(SCHRO_HIP_EXPERIMENTS|SCHRO_HIP_DRY|__HIPCC__|__cplusplus)\b")
    for name in ("hier_bm.hip", "plane_hbm.cpp"):
        path = os.path.join(CSRC, name)
        assert os.path.exists(path), name
        bad = [line for line in open(path) if re.match(r"^\s*#\s*(ifdef|ifndef|if)\b", line) and not allowed.match(line)]
        assert not bad, (name, bad)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "hier_bm.hip" in srcs and "plane_hbm.cpp" in srcs
    # the window scan and the staging are scan_common.h's, not a copy: the block is staged here, the window is staged and
    # scanned by scan_and_store of motion_common.h, which the rough search shares
    text = open(os.path.join(CSRC, "hier_bm.hip")).read()
    common = open(os.path.join(CSRC, "motion_common.h")).read()
    assert '#include "motion_common.h"' in text and "scan_and_store (" in text and "scan_stage_block (" in text
    assert '#include "scan_common.h"' in common and "scan_wave_min (" in common and "scan_stage_window (" in common
    assert "__builtin_amdgcn_alignbyte" not in text and "__builtin_amdgcn_alignbyte" not in common


@pytest.mark.parametrize("lib", ["libschro_hip.so", "libschro_hip_exp.so"])
def test_the_kernel_is_built_without_scratch(lib, tmp_path):
    if not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("no llvm-readelf in this image")
    notes = kernel_notes(os.path.join(ROOT, "schroedinger_amd", lib), tmp_path)
    mine = {n: v for n, v in notes.items() if "hier_bm_kernel" in n}
    assert len(mine) == 1, sorted(mine)
    for n, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] == 0, (n, v)       # (the LDS is sized by the launch)
        assert v["vgpr_count"] <= 128, (n, v)                   # 16 waves of one workgroup on four SIMDs
