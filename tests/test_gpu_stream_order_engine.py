"""The engine's hand-offs under delays (part 2).  The cases are in tests/stream_order_cases.py; they run here in
fresh child processes started with GPU_MAX_HW_QUEUES=8, because their caller's stream must have a window against the
default stream and every stream of the engine, and the four hardware queues a process gets otherwise cannot give it one
(six engine streams and the default stream on four queues).  One child per group of cases that can share a model."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_order_cases.py")
# (cases by number, pytest -k expression, tests the child must pass)
GROUPS = {
    "cases_1_2_3_4_7": ("harness_loop or stage_batched or side_streams or deferred_mode or slow_range_coder", 6 + 1 + 4 + 3 + 6 + 2 + 3),
    "cases_5_8": ("decoder_in_the_loop or whole_sequence", 3 + 1),
    "case_6": ("gop_decode", 8),
}


@pytest.mark.parametrize("group", list(GROUPS))
def test_engine_cases_with_eight_queues(cuda, group):
    expr, count = GROUPS[group]
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    cmd = [sys.executable, "-m", "pytest", CASES, "-m", "gpu", "-x", "-q", "-s", "-p", "no:cacheprovider", "-k", expr]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"{group}: the child ended with status {r.returncode}:\n{r.stdout[-4000:]}"
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == count and "skipped" not in r.stdout.splitlines()[-1], r.stdout.splitlines()[-1]
