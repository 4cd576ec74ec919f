"""The LDS that dd_plan_sweep asks for the registers-in-LDS classes (log2m <= 16): the 64-, 96- and 128-bit window classes
(kclass 1, 3, 2) get 8 KiB behind their k-group's registers for the per-wave raise queues of sweep_kernel (16 waves x 128
records x 4 B; dd_k1.h) while the whole stays within the 80 KiB that keep two workgroups on a CU, and exactly the group's
registers otherwise (the kernel then applies every raise at once); the 32-bit class (kclass 0) never gets a queue and
stays within the 48 KiB of three workgroups per CU."""
import os

import numpy as np
import pytest

os.environ.setdefault("DANDD_NO_TORCH", "1")
from dandd_amd.engine import plan_sweep  # noqa: E402

QUEUE = 16 * 128 * 4
SIZES = [5_000_000, 70_000, 1, 1_000_000]
K_RANGES = [(4, 40), (10, 64), (17, 21), (17, 32), (33, 37), (49, 64), (30, 35), (12, 16), (32, 32)]


@pytest.mark.parametrize("log2m", [8, 10, 12, 13, 14, 15, 16])
@pytest.mark.parametrize("krange", K_RANGES)
def test_lds_of_the_register_classes(log2m, krange):
    m = 1 << log2m
    jobs = plan_sweep(log2m, SIZES, *krange)
    seen = set()
    for kc in np.unique(jobs["kclass"]):
        sel = jobs[jobs["kclass"] == kc]
        lds = {int(v) for v in sel["lds_bytes"]}
        assert len(lds) == 1, "one launch shape per class"
        lds, regs = lds.pop(), int(sel["nk"].max()) * m
        seen.add(int(kc))
        if kc in (1, 2, 3):
            assert lds == (regs + QUEUE if regs + QUEUE <= 80 * 1024 else regs)
            assert lds <= max(80 * 1024, m)
        elif kc == 0:
            assert lds == regs and lds <= max(48 * 1024, m)
    assert seen & {0, 1, 2, 3}


def test_headline_shape_has_queues_and_two_workgroups_per_cu():
    """10 x 50 Mbp, k 4..40, log2m 14: groups of 4 ks = 64 KiB of registers + the queues in the 64- and 96-bit classes."""
    jobs = plan_sweep(14, [50_600_000] * 10, 4, 40)
    for kc in (1, 3):
        sel = jobs[jobs["kclass"] == kc]
        assert set(sel["nk"]) == {4} and set(sel["lds_bytes"]) == {4 * (1 << 14) + QUEUE}
    sel = jobs[jobs["kclass"] == 0]
    assert int(sel["lds_bytes"].max()) == int(sel["nk"].max()) << 14 <= 48 * 1024


def test_a_full_group_leaves_no_room():
    """five ks of the 64-bit class at log2m 14 are one group of 80 KiB: no queue, the kernel's immediate path"""
    jobs = plan_sweep(14, SIZES, 17, 21)
    assert set(jobs["kclass"]) == {1} and set(jobs["nk"]) == {5} and set(jobs["lds_bytes"]) == {80 * 1024}
