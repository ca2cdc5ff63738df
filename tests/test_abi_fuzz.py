"""Every entry point of include/sah_hip.h answers made-up arguments with a status code: tests/abi_fuzz_child.py throws
random extents, pitches, formats, row ranges, device addresses and null sub-pointers at a context that has no device behind it
(sah_debug_create_detached), in a child process so that a fault fails the test instead of ending the run.  CPU only: where a HIP device
exists the hook refuses (the made-up addresses must never reach a GPU) and the test is skipped."""
import pytest

from tests import support


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_no_argument_combination_crashes_an_entry_point(seed):
    support.run_fuzz_child("abi_fuzz_child.py", seed, 1500, timeout=900, tail_lines=25)
