"""The motion-library kernels at their clip, tile and blend edges (tests/motion_edge_cases.py), kernel source on the CPU
emulator.  test_motion_edges_gpu.py runs the same checks on the device."""
import pytest

import motion_edge_cases as E


@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("J", [24, 52])
def test_emu_cook_edge_library_matches_oracle(emu_backend, J, filt):
    E.check_cook(emu_backend, J, filt)


@pytest.mark.parametrize("J", [24, 52])
def test_emu_blended_lookup_at_frame_boundaries_and_slerp_branches(emu_backend, J):
    E.check_blended_edges(emu_backend, J)


@pytest.mark.parametrize("J", [24, 52])
def test_emu_intervaled_lookup_is_the_gather_of_the_oracle_frame(emu_backend, J):
    E.check_intervaled_edges(emu_backend, J)


def test_emu_masked_lookup_null_outputs_and_guard_rows(emu_backend):
    E.check_masked_lookup(emu_backend)


def test_emu_resample_is_bit_exact(emu_backend):
    E.check_resample(emu_backend)


@pytest.mark.parametrize("J,n", [(24, 1), (24, 2), (24, 9), (52, 1), (52, 5)])
def test_emu_imitation_step_edges(emu_backend, J, n):
    E.check_imitation_edges(emu_backend, J, n)
