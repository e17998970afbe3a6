"""The fused optimizer's bits against a recorded run: tests/golden/optim_step_sha256.json holds, per case of
tests/golden/gen_optim_digests.py, the SHA-256 of everything three steps of FusedAdamW / FusedLamb leave behind
(parameters, moments, EMA, shadows, trust ratios, clip state), recorded at the commit before the step paths were
merged into one.  The existing tests compare the optimizer with itself (grouped against per-group) or with fp64 under a
tolerance; neither would notice a host factor that is now rounded differently.  `fuse_groups` off and on must both
give the one recorded digest."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_optim_digests", os.path.join(GOLDEN, "gen_optim_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "optim_step_sha256.json")) as f:
    RECORDED = json.load(f)


def test_every_case_of_the_generator_is_recorded():
    assert sorted(RECORDED["digests"]) == sorted(gen.CASES)


@pytest.mark.parametrize("case", gen.CASES)
def test_three_steps_leave_the_recorded_bits(case):
    want = RECORDED["digests"][case]
    for fuse in (False, True):
        got = gen.digest(case, fuse)
        assert got == want, (f"{case} with fuse_groups={fuse}: digest {got}, recorded {want}; recorded under "
                             f"{RECORDED['toolchain']}, this run under {gen.toolchain()}")
