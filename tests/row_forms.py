"""The OBMC row kernels as the sources declare them, and the pictures that reach each one (host side: no GPU needed).

obmc_row.hip (half / quarter pel), obmc_row_plain.hip (full pel) and obmc_row_eighth.hip (eighth pel) each instantiate
their kernels with SCHRO_ROW_KERNEL (name, waves, <obmc_row_body's template arguments>) and end with a table of
ROW_ENTRY (name) lines; row_kernel (const RowForm &) takes the entry whose form matches, else -- for a prediction-only
launch -- the entry of the same form with the residual.  parse () reads both; case_for (form) names a picture (make_case's
arguments) with a plane of that form.

The admission side: obmc_row_form (obmc_row.hip) decides which planes the row kernels take.  admission_program () compiles
its own text -- from the row length to the table capacities -- with RowGeo (obmc_row_body.h) into a host program that
answers for a list of block geometries and prints the kernels' table capacities; enumerate_geometries () walks every
geometry schro_params_verify_block_params allows (plane_obmc.cpp) and counts, by brute force over block footprints, what
meets one tile."""
import collections
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schroedinger_amd", "csrc")
SOURCES = {1: "obmc_row.hip", 0: "obmc_row_plain.hip", 3: "obmc_row_eighth.hip"}

# (kind: 0 plain planes, 1 half-pel images at half / quarter pel, 3 at eighth pel; nd: dwords per row and segment; np: planes
# per job, 3 = (U, V) pairs; ns: segments per block row; nores: prediction-only; weighted: weights other than 1, 1 / 2)
Form = collections.namedtuple("Form", "kind nd np ns nores weighted")
Kernel = collections.namedtuple("Kernel", "name form source experiments")

# obmc_row_body.h: row_form < ND, NP, UV = false, TH = kRTH, NORES = false, RK = 1, NS = 1, WP = false, PAD = false >
_DEFAULTS = ["", "", "false", "kRTH", "false", "1", "1", "false", "false"]
# a switch of the experiments library that is the only way to a kernel (obmc_row.hip: row_kernel)
EXPERIMENT_SWITCHES = {"obmc_row_kernel_p_3_1_pad": {"SCHRO_HIP_OBMC_PAD": "1"}}


def _form_of(args, kind_of_file):
    a = [s.strip() for s in args.split(",")]
    a += _DEFAULTS[len(a):]
    nd, np_, uv, _, nores, rk, ns, wp, _ = a
    b = lambda s: {"true": True, "false": False}[s]
    rk = int(rk)
    assert rk == kind_of_file, (args, kind_of_file)
    return Form(rk, int(nd), 3 if b(uv) else int(np_), int(ns), b(nores), b(wp))


@functools.lru_cache(None)
def parse():
    """{name: Kernel} of every SCHRO_ROW_KERNEL; a kernel of no ROW_ENTRY table is an experiments build's (under
    #ifdef SCHRO_HIP_EXPERIMENTS) -- see EXPERIMENT_SWITCHES."""
    out = {}
    for kind, src in SOURCES.items():
        text = open(os.path.join(CSRC, src)).read()
        table = re.search(r"constexpr RowEntry k\w+\[\] = \{(.*?)\};", text, re.S).group(1)
        entries = re.findall(r"ROW_ENTRY \((\w+)\)", table)
        assert len(entries) == len(set(entries)), src
        exp_spans = [(m.start(), m.end()) for m in re.finditer(r"#ifdef SCHRO_HIP_EXPERIMENTS.*?#endif", text, re.S)]
        for m in re.finditer(r"^SCHRO_ROW_KERNEL \((\w+), \d+, (.*)\)\s*$", text, re.M):
            name = m.group(1)
            exp = any(a <= m.start() < b for a, b in exp_spans)
            assert (name in entries) != exp, "%s: in a table xor under the experiments switch" % name
            assert name not in out, name
            out[name] = Kernel(name, _form_of(m.group(2), kind), src, exp)
        assert set(entries) <= set(out), (src, set(entries) - set(out))
    return out


def table_kernels():
    """The kernels of the three tables (what the product library's row_kernel can pick)."""
    return {n: k for n, k in parse().items() if not k.experiments}


def row_find(form):
    """row_kernel's rule: the entry of the form, else for a prediction-only form the entry of its residual twin."""
    by_form = {k.form: k.name for k in table_kernels().values()}
    if form in by_form:
        return by_form[form]
    if form.nores:
        return by_form.get(form._replace(nores=False))
    return None


def pairs_pay_tiles(cus):
    """Chroma tiles (128 x 32) of row-kernel planes a call must carry for its U + V planes to merge into two-plane jobs
    (plane_obmc.cpp: pairs_pay, more than six per CU)."""
    return 6 * cus + 1


# Component block lengths (pixels; (U, V) pairs: samples) of each row length: (nd, ns) -> (plane xblen, uv xblen)
_ROW = {(2, 1): (8, 4), (3, 1): (12, 6), (4, 1): (16, 8), (3, 2): (24, 12), (4, 2): (32, 16)}
# luma block sets (xblen, xbsep) whose 4:2:0 chroma has a given length: chroma xblen -> luma set
_LUMA_FOR_CHROMA = {4: (8, 4), 6: (12, 8), 8: (16, 12), 12: (24, 16), 16: (32, 16)}
_LUMA_SET = {8: (8, 4), 12: (12, 8), 16: (16, 12), 24: (24, 16), 32: (32, 16)}
# Full pel, two-plane jobs: at full pel a picture's U and V planes become one (U, V) job wherever obmc_row_form takes them as
# one (plane_obmc.cpp: uv_plain), and no block geometry fits a plane's tables but not a (U, V) job's
# (tests/test_row_forms.py: test_full_pel_two_plane_forms_need_the_pair_tile_limit).  What is left is the tile count: a
# (U, V) job's tiles are 64 pixels wide, so 16384 x 8192 4:4:4 chroma planes are 65 536 (U, V) tiles -- over the order
# table's 16 bits -- and 32 768 plane tiles: the planes go out as two-plane jobs.  (nd -> block set)
FULLPEL_TWO_PLANE = dict(w=16384, h=8192, chroma=(0, 0))
_FULLPEL_TWO_PLANE_SET = {2: (8, 4), 3: (12, 8), 4: (16, 12)}


def case_for(form, cus=None, prec=None):
    """make_case's keyword arguments (w, h, xblen, xbsep, prec, weights, chroma, mv_range, + extras) of a picture with a plane
    of `form`; two-plane jobs need a call over pairs_pay (cus: the device's compute units), which the picture carries on
    its own.  `component` (not make_case's) names the plane that takes the form (the U plane of a (U, V) or two-plane
    job)."""
    if prec is None:
        prec = {0: 0, 1: 2, 3: 3}[form.kind]
    assert {0: (0,), 1: (1, 2), 3: (3,)}[form.kind].count(prec), (form, prec)
    plane_len, uv_len = _ROW[(form.nd, form.ns)]
    weights = (3, 5, 3) if form.weighted else (1, 1, 1)
    a = dict(prec=prec, weights=weights, mv_range=40 << prec, prediction_only=1 if form.nores else 0)
    if form.np == 1:
        a.update(chroma=(1, 1), component=0)
        a["xblen"], a["xbsep"] = _LUMA_SET[plane_len]
    elif form.np == 3:
        # (U, V) jobs: pair images, at full pel the two plain planes of each reference
        a.update(chroma=(1, 1), component=1, pair=prec > 0)
        a["xblen"], a["xbsep"] = _LUMA_FOR_CHROMA[uv_len]
    else:
        assert form.np == 2 and not form.weighted
        assert cus is not None, "two-plane jobs: the threshold depends on the device's compute units"
        a.update(component=1)
        assert form.ns == 1
        if form.kind == 0:
            a.update(FULLPEL_TWO_PLANE, only=(1, 2), residual=form.nores)
            a["xblen"], a["xbsep"] = _FULLPEL_TWO_PLANE_SET[form.nd]
        else:
            # one-component half-pel images, 4:4:4: the U and V planes stay plane jobs and merge where the call pays --
            # 2048 pixels wide, as many tile rows as take the two planes over the threshold
            a.update(chroma=(0, 0), pair=False, w=2048, h=32 * (-(-pairs_pay_tiles(cus) // 32) + 1))
            a["xblen"], a["xbsep"] = _LUMA_SET[plane_len]
    if a["xbsep"] == 4:
        # (8 / 4 blocks that are also 8 / 4 high meet more rows of a tile than the 8-byte kernels' items hold: obmc.hip)
        a.update(yblen=16, ybsep=12)
    a.setdefault("w", 96)
    a.setdefault("h", 64)
    return a


def chroma_pair_tiles(a):
    """The 128 x 32 tiles of a picture's two chroma planes (what plane_obmc.cpp's pairs_pay counts)."""
    cw, ch = -(-a["w"] // (1 << a["chroma"][0])), -(-a["h"] // (1 << a["chroma"][1]))
    return 2 * ((cw + 127) // 128) * ((ch + 31) // 32)


# ---- the admission, compiled from its source, and the brute force it is checked by --------------------------------

def _extract(text, start, end):
    i = text.index(start)
    return text[i:text.index(end, i)]


def admission_program(out_dir):
    """Builds and returns the path of a host program made of obmc_row_form's text from the row length on (its pointer and
    kernel checks answered by stubs: aligned references, every form has a kernel) and of obmc_row_body.h's RowGeo.  It
    reads lines "xblen yblen xbsep ybsep uv" and prints "nd ns" (0 0: refused); argument "caps" prints
    "nd ns uv tw blk item" for every class instead."""
    body = open(os.path.join(CSRC, "obmc_row_body.h")).read()
    row = open(os.path.join(CSRC, "obmc_row.hip")).read()
    rth = re.search(r"constexpr int kRTH = \d+;", body).group(0)
    geo = _extract(body, "template < int ND, bool UV, int NS = 1 > struct RowGeo {", "\n};") + "\n};\n"
    caps = _extract(row, "struct RowCaps {", "// The form of the row kernel")
    form_fn = _extract(row, "RowForm\nobmc_row_form (const ObmcJob & j, bool uv, bool nores)\n{", "\n}\n") + "\n}\n"
    # (what the geometry does not decide: references aligned, every form has a kernel)
    form_fn = form_fn.replace("if (!row_kernel (form))", "if (false)")
    src = r"""#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iterator>
#include <cstring>
namespace schro {
%(rth)s
constexpr int kHpApron = 32;
static int hp_chunks (int w, int ps = 0) { return (((w + 2 * kHpApron) << ps) + 15) / 16 + 1; }
struct RowForm {
  int kind, nd, np, ns;
  bool nores, weighted;
  constexpr explicit operator bool () const { return nd != 0; }
};
struct ObmcJob {
  int w, h, xblen, yblen, xbsep, ybsep, xoff, yoff, prec, w1, w2, wbits, ref_ps;
  const void *ref[2], *ref_b[2];
  int ref_stride[2];
};
%(geo)s
%(caps)s
%(form_fn)s
}
using namespace schro;
int main (int argc, char **argv)
{
  if (argc > 1 && !strcmp (argv[1], "caps")) {
    for (int uv = 0; uv < 2; uv++)
      for (int ns = 1; ns <= 2; ns++)
        for (int nd = 2; nd <= 4; nd++) {
          const RowCaps c = row_caps (nd, ns, uv);
          printf ("%%d %%d %%d %%d %%d %%d\n", nd, ns, uv, c.tw, c.blk, c.item);
        }
    return 0;
  }
  alignas (128) static char buf[4096];
  int xblen, yblen, xbsep, ybsep, uv;
  // a plane of 1024 x 1024 at half pel: whole tiles, origins and tile counts far inside their limits
  while (scanf ("%%d %%d %%d %%d %%d", &xblen, &yblen, &xbsep, &ybsep, &uv) == 5) {
    ObmcJob j = {};
    j.w = j.h = 1024;
    j.xblen = xblen, j.yblen = yblen, j.xbsep = xbsep, j.ybsep = ybsep;
    j.xoff = (xblen - xbsep) / 2, j.yoff = (yblen - ybsep) / 2;
    j.prec = 1, j.w1 = j.w2 = j.wbits = 1, j.ref_ps = uv;
    j.ref[0] = j.ref[1] = j.ref_b[0] = j.ref_b[1] = buf;
    j.ref_stride[0] = j.ref_stride[1] = hp_chunks (j.w, uv) * 512;
    const RowForm f = obmc_row_form (j, uv != 0, false);
    printf ("%%d %%d\n", f.nd, f.ns);
  }
  return 0;
}
""" % dict(rth=rth, geo=geo, caps=caps, form_fn=form_fn)
    src = src.replace("__host__ __device__ ", "")
    path = os.path.join(out_dir, "row_admission.cpp")
    with open(path, "w") as f:
        f.write(src)
    exe = os.path.join(out_dir, "row_admission")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", path, "-o", exe],
                   check=True)
    return exe


def run_admission(exe, geos):
    """[(xblen, yblen, xbsep, ybsep, uv)] -> [(nd, ns)] (nd 0: refused)."""
    p = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % g for g in geos), capture_output=True, text=True,
                       check=True)
    rows = [tuple(map(int, ln.split())) for ln in p.stdout.split("\n") if ln]
    assert len(rows) == len(geos)
    return rows


def read_caps(exe):
    """{(nd, ns, uv): (tw, blk, item)} as RowGeo declares them."""
    p = subprocess.run([exe, "caps"], capture_output=True, text=True, check=True)
    out = {}
    for ln in p.stdout.split("\n"):
        if ln:
            nd, ns, uv, tw, blk, item = map(int, ln.split())
            out[(nd, ns, bool(uv))] = (tw, blk, item)
    return out


def luma_geometries():
    """Every luma (xblen, xbsep) of schro_params_verify_block_params (plane_obmc.cpp): multiples of 4, sep <= len <= 2 sep,
    len <= 64."""
    return [(blen, sep) for sep in range(4, 65, 4) for blen in range(sep, min(2 * sep, 64) + 1, 4)]


@functools.lru_cache(None)
def axis_counts(blen, sep, tile, seg):
    """Brute force along one axis, over every phase of the tile against the block grid (blocks start at i sep - off, off =
    (blen - sep) / 2; the tile at [t, t + tile) for t = 0 .. sep - 1 -- and every later tile is one of these).  For each
    phase: the blocks whose footprint meets the tile, and the samples of the tile covered by block SEGMENTS of length
    `seg` that meet it, summed over those segments (along x: blocks are cut into blen / seg segments; along y: seg = blen).
    Returns (max blocks, max covered samples)."""
    off = (blen - sep) // 2
    best_n = best_cov = 0
    for t in range(sep):
        n = cov = 0
        # (blocks from far in front of the tile to far behind it; the grid is unbounded: the interior of a plane)
        for i in range(-(2 * tile + 2 * blen) // sep - 2, (2 * tile + 2 * blen) // sep + 2):
            b0 = i * sep - off
            if b0 + blen <= t or b0 >= t + tile:
                continue
            n += 1
            for s in range(blen // seg):
                s0 = b0 + s * seg
                lo, hi = max(s0, t), min(s0 + seg, t + tile)
                cov += max(0, hi - lo)
        best_n, best_cov = max(best_n, n), max(best_cov, cov)
    return best_n, best_cov


def brute_counts(xblen, yblen, xbsep, ybsep, ns, tw, th):
    """What one tile of tw x th meets, worst phase: block records (every segment of a block that meets the tile: the
    kernel's table holds them all), the segments per block row (nbi) and the (segment, row) items -- rows of segments
    that overlap the tile horizontally and lie in its rows."""
    seg = xblen // ns
    nx, _ = axis_counts(xblen, xbsep, tw, seg)
    ny, rows = axis_counts(yblen, ybsep, th, yblen)
    # items: per segment that meets the tile, its rows inside it; the x count is of segments, which differs from nx * ns
    # when a block's segment lies beside the tile
    segs_x = _segments_meeting(xblen, xbsep, tw, seg)
    return dict(blk=nx * ns * ny, nbi=nx * ns, nbj=ny, item=segs_x * rows)


@functools.lru_cache(None)
def _segments_meeting(blen, sep, tile, seg):
    off = (blen - sep) // 2
    best = 0
    for t in range(sep):
        n = 0
        for i in range(-(2 * tile + 2 * blen) // sep - 2, (2 * tile + 2 * blen) // sep + 2):
            b0 = i * sep - off
            for s in range(blen // seg):
                s0 = b0 + s * seg
                if s0 + seg > t and s0 < t + tile:
                    n += 1
        best = max(best, n)
    return best


def enumerate_geometries(exe):
    """Every component geometry of every legal luma geometry and chroma subsampling (hs, vs in 0, 1), as a plane (uv False)
    and as the U plane of a (U, V) job: [dict(geo, uv, luma, shift, nd, ns, counts, caps)] -- nd 0: refused by
    obmc_row_form."""
    lg = luma_geometries()
    geos = {}
    for hs in (0, 1):
        for vs in (0, 1):
            for xb, xs in lg:
                for yb, ys in lg:
                    g = (xb >> hs, yb >> vs, xs >> hs, ys >> vs)
                    for uv in (False, True):
                        geos.setdefault(g + (uv,), ((xb, xs, yb, ys), (hs, vs)))
    keys = sorted(geos)
    answers = run_admission(exe, [k[:4] + (int(k[4]),) for k in keys])
    caps = read_caps(exe)
    th = int(re.search(r"constexpr int kRTH = (\d+);", open(os.path.join(CSRC, "obmc_row_body.h")).read()).group(1))
    out = []
    for k, (nd, ns) in zip(keys, answers):
        xblen, yblen, xbsep, ybsep, uv = k
        rec = dict(geo=k[:4], uv=uv, luma=geos[k][0], shift=geos[k][1], nd=nd, ns=ns)
        # the class a refused geometry would have had (its row length) -- for the refused geometries of a class
        seg_bytes = xblen << (1 if uv else 0)
        cns = 2 if seg_bytes > 16 else 1
        cnd = max(2, (seg_bytes // cns + 3) // 4)
        rec["class"] = (nd, ns, uv) if nd else ((cnd, cns, uv) if seg_bytes <= 32 and (seg_bytes <= 16 or seg_bytes % 4 == 0)
                                                 and yblen <= 32 else None)
        if rec["class"] is not None:
            tw, blk, item = caps[rec["class"]]
            rec["caps"] = dict(tw=tw, blk=blk, item=item, th=th)
            rec["counts"] = brute_counts(xblen, yblen, xbsep, ybsep, rec["class"][1], tw, th)
        out.append(rec)
    return out, caps, th


def limit_geometries(recs):
    """For each (nd, ns, uv) class: the admitted geometry closest to each capacity (blk, item, nbi), and ("refused") among the
    refused geometries whose brute-force counts exceed a capacity the one with the smallest load over it.  obmc_row_form's
    bound is an upper bound of those counts, so the geometry where it starts to refuse may still fit the tables: that one
    is a different geometry, and such geometries are not rendered."""
    by_class = collections.defaultdict(dict)
    for r in recs:
        c = r.get("class")
        if c is None:
            continue
        load = max(r["counts"]["blk"] / r["caps"]["blk"], r["counts"]["item"] / r["caps"]["item"], r["counts"]["nbi"] / 255)
        slot = by_class[c]
        if r["nd"]:
            for cap in ("blk", "item", "nbi"):
                v = r["counts"][cap] / (255 if cap == "nbi" else r["caps"][cap])
                if cap not in slot or v > slot[cap][0]:
                    slot[cap] = (v, r)
        elif load > 1 and ("refused" not in slot or load < slot["refused"][0]):
            slot["refused"] = (load, r)
    return {c: {k: v[1] for k, v in s.items()} for c, s in by_class.items()}


# ---- both sides of each admission limit --------------------------------------------------------------------------

def origin_limit(prec):
    """The largest max (w, h) whose rim origins fit 16 bits at this precision: ((max (w, h) + 32) << prec) <= 32767."""
    return (32767 >> prec) - 32


def _far(prec, size):
    # vectors as long as the int16 field carries, at most the plane and its margin: rim blocks clamp to both extremes
    return min(32767, (size + 64) << prec) // 2


def limit_cases():
    """[(limit, side, spec)]: side "admitted" -- every rendered plane goes to a row kernel -- or "refused" -- none does
    (obmc.hip), or "error" -- the call is refused.  spec: make_case's keyword arguments; `only` the components rendered;
    ref_offset / ref_stride_pad (full pel): the references' pointer / row stride off by that many bytes; big: a picture
    of 2^28 samples (the tile limit).  The capacity cases are the host enumeration's (capacity_cases)."""
    out = []
    for prec in range(4):
        m = origin_limit(prec)
        for side, size in (("admitted", m), ("refused", m + 1)):
            for axis in ("w", "h"):
                w, h = (size, 40) if axis == "w" else (40, size)
                out.append(("origin_p%d_%s%d" % (prec, axis, size), side,
                            dict(w=w, h=h, xblen=12, xbsep=8, prec=prec, weights=(1, 1, 1), chroma=(1, 1), only=(0,),
                                 mv_range=_far(prec, size))))
    # tiles: 65 535 luma tiles (255 x 257 of 128 x 32) against 65 536 (128 x 512), full pel; and (U, V) jobs' 64-pixel tiles:
    # 65 535 (255 x 257) -- the 65 536 of FULLPEL_TWO_PLANE go out as two-plane jobs (test_every_form)
    out.append(("tiles_luma_65535", "admitted", dict(w=32640, h=8224, xblen=12, xbsep=8, prec=0, weights=(1, 1, 1), chroma=(1, 1),
                                                     only=(0,), mv_range=40, residual=False, big=True)))
    out.append(("tiles_luma_65536", "refused", dict(w=16384, h=16384, xblen=12, xbsep=8, prec=0, weights=(1, 1, 1), chroma=(1, 1),
                                                    only=(0,), mv_range=40, residual=False, big=True)))
    out.append(("tiles_uv_65535", "admitted", dict(w=16320, h=8224, xblen=8, xbsep=4, prec=0, weights=(1, 1, 1), chroma=(0, 0),
                                                   only=(1, 2), mv_range=40, residual=False, big=True)))
    # yblen 32 against 36; rows of 32 against 36 bytes (luma 32 / 36 pixels; (U, V) 16 / 18 samples of pair images)
    out.append(("yblen_32", "admitted", dict(w=200, h=136, xblen=12, xbsep=12, yblen=32, ybsep=16, prec=2, weights=(1, 1, 1),
                                             chroma=(1, 1), only=(0,), mv_range=80)))
    out.append(("yblen_36", "refused", dict(w=200, h=136, xblen=12, xbsep=12, yblen=36, ybsep=20, prec=2, weights=(1, 1, 1),
                                            chroma=(1, 1), only=(0,), mv_range=80)))
    for prec in (0, 2):
        # (blocks 12 high: a block as high as it is long would be refused for its height, yblen > 32, first)
        out.append(("row_32_bytes_p%d" % prec, "admitted", dict(w=300, h=100, xblen=32, xbsep=16, yblen=12, ybsep=8, prec=prec,
                                                                weights=(1, 1, 1), chroma=(1, 1), only=(0,), mv_range=40 << prec)))
        out.append(("row_36_bytes_p%d" % prec, "refused", dict(w=300, h=100, xblen=36, xbsep=20, yblen=12, ybsep=8, prec=prec,
                                                               weights=(1, 1, 1), chroma=(1, 1), only=(0,), mv_range=40 << prec)))
    out.append(("uv_row_32_bytes", "admitted", dict(w=300, h=100, xblen=32, xbsep=16, prec=2, weights=(1, 1, 1), chroma=(1, 1),
                                                    only=(1, 2), pair=True, mv_range=80)))
    out.append(("uv_row_36_bytes", "refused", dict(w=300, h=100, xblen=36, xbsep=20, prec=2, weights=(1, 1, 1), chroma=(1, 1),
                                                   only=(1, 2), pair=True, mv_range=80)))
    # weights: bits 6 (the most the library takes), a zero weight -- admitted; a negative weight -- refused; bits 7 -- an error
    for prec in (0, 2):
        for name, side, wt in (("wbits_6", "admitted", (21, 43, 6)), ("weight_zero", "admitted", (0, 64, 6)),
                               ("weight_zero_2", "admitted", (8, 0, 3)), ("weight_negative", "refused", (-1, 65, 6)),
                               ("wbits_7", "error", (42, 86, 7))):
            out.append(("%s_p%d" % (name, prec), side, dict(w=136, h=72, xblen=12, xbsep=8, prec=prec, weights=wt, chroma=(1, 1),
                                                            pair=prec > 0, mv_range=40 << prec)))
    # full-pel alignment: references of whole dwords and w >= 4
    base = dict(w=136, h=72, xblen=12, xbsep=8, prec=0, weights=(1, 1, 1), chroma=(1, 1), mv_range=40)
    out.append(("align_dword", "admitted", dict(base, ref_offset=4, ref_stride_pad=4)))
    for k in (1, 2, 3):
        out.append(("align_stride_%d" % k, "refused", dict(base, ref_stride_pad=k)))
        out.append(("align_pointer_%d" % k, "refused", dict(base, ref_offset=k)))
    # (U, V) jobs of 4:2:2 chroma 4 and 3 pixels wide (luma 8 and 6, 4 / 4 blocks: 2 / 4 chroma blocks -- 4:2:0's 2 / 2 meet
    # more blocks of a tile than the tables hold)
    out.append(("width_4", "admitted", dict(w=8, h=64, xblen=4, xbsep=4, prec=0, weights=(1, 1, 1), chroma=(1, 0), only=(1, 2),
                                            mv_range=24)))
    out.append(("width_3", "refused", dict(w=6, h=64, xblen=4, xbsep=4, prec=0, weights=(1, 1, 1), chroma=(1, 0), only=(1, 2),
                                           mv_range=24)))
    return out


def capacity_cases(limits):
    """limit_geometries' geometries as pictures: [(name, side, spec)].  A plane class renders the component of that geometry
    from one-component quarter-pel images (the U and V planes stay plane jobs); a (U, V) class the chroma planes of pair
    images, or of full-pel planes where the chroma is not subsampled horizontally (pair images are of 4:2:x chroma) -- every
    refused (U, V) geometry is of 4:2:x chroma (asserted): its planes must not fall back to the plane forms."""
    out = []
    seen = set()
    for (nd, ns, uv), slot in sorted(limits.items()):
        for which, r in sorted(slot.items()):
            side = "refused" if which == "refused" else "admitted"
            key = (r["geo"], uv, side)
            if key in seen:
                continue
            seen.add(key)
            (xb, xs, yb, ys), (hs, vs) = r["luma"], r["shift"]
            comp = (0,) if (hs, vs) == (0, 0) and not uv else (1, 2)
            chroma = (hs, vs) if comp != (0,) else (1, 1)
            assert not (uv and side == "refused") or hs == 1, r
            prec = 0 if uv and hs == 0 else 2
            # a plane wide and high enough for several tiles of every phase
            w, h = (520 << hs, 200 << vs) if comp != (0,) else (520, 200)
            out.append(("cap_%s_nd%d_ns%d_%s_%dx%d_%dx%d_c%d%d" % (which, nd, ns, "uv" if uv else "plane", xb, yb, xs, ys, hs, vs),
                        side, dict(w=w, h=h, xblen=xb, xbsep=xs, yblen=yb, ybsep=ys, prec=prec, weights=(1, 1, 1), chroma=chroma,
                                   only=comp, pair=uv and prec > 0, mv_range=40 << prec)))
    return out
