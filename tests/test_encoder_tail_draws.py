"""CPU: the draws of the encoder tail's GPU tests are what their docstrings promise (tests/dry_run_encoder_tail_cases.py walks
tests/encoder_tail_draws.py with the Python checkers, no device), and the seconds each test spends in the checkers are
printed (`pytest -s`): recorded, not asserted."""
import pytest

import dry_run_encoder_tail_cases as W
from test_gpu_iwt_forward import pixel_range


@pytest.mark.parametrize("name", list(W.MEASURED))
def test_draws_cover_what_the_docstrings_promise(name):
    walk = {"test_lowdelay_encode_random_pictures": W.walk_lowdelay, "test_quantise_random_codeblocks": W.walk_quantise,
            "test_histogram_random_bands": W.walk_histogram, "test_chain_on_the_plane_layer": lambda: W.walk_chain(pixel_range)}[name]
    spent, facts = walk()
    print("%s: %.2f s in the checkers (%.1f when the counts were set) %s" % (name, spent, W.MEASURED[name], facts))
