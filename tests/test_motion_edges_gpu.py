"""The motion-library kernels at their clip, tile and blend edges (tests/motion_edge_cases.py) on the device: what the
emulator cannot see is the -O3 build with its contraction and the device's acosf / atan2f / sinf, the wave-level LDS hand-off,
the dynamic-LDS sizing of the velocity kernel, grid rounding and the shuffle ladders over 32- and 64-lane groups."""
import pytest

import motion_edge_cases as E

pytestmark = pytest.mark.gpu


def _lib():
    from smplsim_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("J", [24, 52])
def test_gpu_cook_edge_library_matches_oracle(J, filt):
    E.check_cook(_lib(), J, filt)


@pytest.mark.parametrize("J", [24, 52])
def test_gpu_blended_lookup_at_frame_boundaries_and_slerp_branches(J):
    E.check_blended_edges(_lib(), J)


@pytest.mark.parametrize("J", [24, 52])
def test_gpu_intervaled_lookup_is_the_gather_of_the_oracle_frame(J):
    E.check_intervaled_edges(_lib(), J)


def test_gpu_masked_lookup_null_outputs_and_guard_rows():
    E.check_masked_lookup(_lib())


def test_gpu_resample_is_bit_exact():
    E.check_resample(_lib())


@pytest.mark.parametrize("J,n", [(24, 1), (24, 2), (24, 9), (52, 1), (52, 5)])
def test_gpu_imitation_step_edges(J, n):
    E.check_imitation_edges(_lib(), J, n)
