"""The rate controller restated from its definition, independently of pmctf_rate: the yardstick of
tests/test_rate_control_cpu.py and tests/test_gpu_rate_control.py.  Plain integers; sizes come from a table or a callable.
Nothing here is imported from pmctf_rate, and nothing here checks its arguments."""
from fractions import Fraction


def fps_fraction(fps):
    return Fraction(fps[0], fps[1]) if isinstance(fps, (tuple, list)) else Fraction(fps, 1)


def allocations(sizes, bitrate, fps):
    """floor(size * bitrate / fps) per GOP, fps a rational"""
    f = fps_fraction(fps)
    out = []
    for size in sizes:
        exact = Fraction(size * bitrate) / f
        out.append(exact.numerator // exact.denominator)
    return out


def choose(size_of, choices, start, budget, max_trials, slack):
    """-> (index accepted, fits, bits, [(q, bits)] tried in order)"""
    tried = []

    def go(i):
        b = size_of(choices[i])
        tried.append((choices[i], b))
        return b

    first = go(start)
    if first <= budget:                                              # climb
        best_i, best_b = start, first
        while True:
            if best_i == len(choices) - 1:
                break
            if len(tried) == max_trials:
                break
            if not best_b < (1 - slack) * budget:
                break
            b = go(best_i + 1)
            if b <= budget:
                best_i, best_b = best_i + 1, b
            else:
                break
        return best_i, True, best_b, tried
    i, b = start, first                                              # descend
    while i >= 1 and len(tried) < max_trials:
        i -= 1
        b = go(i)
        if b <= budget:
            return i, True, b, tried
    return i, False, b, tried


def run(sizes, size_of, bitrate, fps, q_choices, q_start=None, bucket_ms=1000, max_trials=4, slack=0.0):
    """-> the records of run_controller: [{"alloc", "budget", "q_index", "fits", "bits", "trials", "credit"}]"""
    choices = list(q_choices)
    at = len(choices) // 2 if q_start is None else choices.index(q_start)
    bucket = bitrate * bucket_ms // 1000
    credit = 0
    out = []
    for k, alloc in enumerate(allocations(sizes, bitrate, fps)):
        budget = alloc + credit
        at, fits, bits, tried = choose(lambda q: size_of(k, q), choices, at, budget, max_trials, slack)
        credit = credit + alloc - bits
        if credit > bucket:
            credit = bucket
        out.append({"alloc": alloc, "budget": budget, "q_index": choices[at], "fits": fits, "bits": bits, "trials": tried,
                    "credit": credit})
    return out
