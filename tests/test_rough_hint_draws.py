"""CPU: what the named cases and the 30 random draws of tests/test_gpu_rough_hint.py cover -- every skip reason of the
candidate test, blocks of no size with a valid window (inside and outside of which the gravity position lies) and with an
invalid one, diagonals longer than the workgroup has waves, every shift, both references, aprons, padded strides."""
import numpy as np

import rough_hint_cases as K
import rough_hint_draws as D
import schroedinger_amd as sa


def test_the_wave_count_is_the_headers():
    assert K.ROUGH_WAVES == sa.ROUGH_WAVES


def test_named_cases_cover_what_they_are_there_for():
    both = 0
    for name in K.CASES:
        field, stats = K.expected(name)         # (asserts the case's own `want`)
        assert field.size == K.CASES[name]["nbx"] * K.CASES[name]["nby"]
        both += stats["empty_block_scan"] > 0 and stats["invalid_window"] > 0
    assert both >= 1
    assert {c["shift"] for c in K.CASES.values()} == {1, 2, 3}
    assert {c["ref_index"] for c in K.CASES.values()} == {0, 1} and {c["ext"] for c in K.CASES.values()} == {0, 32}
    assert {(c["xb"], c["yb"]) for c in K.CASES.values()} >= {(8, 8), (12, 12), (16, 16), (16, 8), (4, 4), (64, 64)}
    assert all(c["w"] <= 100 and c["h"] <= 80 for n, c in K.CASES.items() if n != "long_diagonal")


def test_random_draws_cover_every_path():
    total, shifts, refs, exts, npics, pads = {}, set(), set(), set(), set(), set()
    inside = 0
    for n in range(D.N_DRAWS):
        pics = D.draw(n)
        npics.add(len(pics))
        for c, (field, stats) in zip(pics, D.expected(n)):
            for k, v in stats.items():
                total[k] = total.get(k, 0) + int(v)
            inside += stats["empty_block_scan"] - stats["gravity_outside"]
            shifts.add(c["shift"]), refs.add(c["ref_index"]), exts.add(c["ext"]), pads.add(c["pad"] > 0)
            assert np.abs(c["hint"]["v"]).max() > 0
    for key in ("skip_negative", "skip_empty", "skip_beyond", "all_skipped", "invalid_window", "empty_block_scan", "gravity_outside", "turns"):
        assert total[key] > 0, (key, total)
    assert inside > 0
    assert shifts == {1, 2, 3} and refs == {0, 1} and exts == {0, 8, 32} and npics == {1, 2, 3} and pads == {True, False}
    # the draws are the same in every process
    assert D.draw(3)[0]["frame"].tobytes() == D.draw.__wrapped__(3)[0]["frame"].tobytes()
