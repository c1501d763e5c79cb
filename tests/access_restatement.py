"""Which files a picture of a GOP depends on, restated as the dataflow of pmctf_gop.decode_gop_files + decode_gop with sets of
file names instead of tensors: no formula of pmctf_access.gop_plan is used.  The yardstick of tests/test_random_access_cpu.py."""


def coding_order(size):
    """[(stage, i_ref, i_cur)] as encode_gop codes the pairs: stage by stage, each stage left to right"""
    out, stage, step = [], 0, 1
    while step < size:
        out += [(stage, i_ref, i_ref + step) for i_ref in range(0, size, 2 * step)]
        stage, step = stage + 1, 2 * step
    return out


def all_files(size):
    """every file of the GOP in the order it is written"""
    names = []
    for _, _, i_cur in coding_order(size):
        names += [f"{i_cur}.bin", f"{i_cur}_C_main.bin", f"{i_cur}_mv.bin"]
    return names + ["0_main.bin", "0_C_main.bin"]


def closure(size, wanted):
    """the files the pictures `wanted` of a GOP of `size` depend on, in all_files order"""
    pairs = coding_order(size)
    # what decode_gop_files decodes: every coded entry from its two picture files ...
    entry = [None] * size
    entry[0] = {"0_main.bin", "0_C_main.bin"}
    for _, _, i_cur in pairs:
        entry[i_cur] = {f"{i_cur}.bin", f"{i_cur}_C_main.bin"}
    # ... and every motion from its own file and the previous motion of its stage (the context restarts per stage)
    motion, at_stage, before = {}, None, set()
    for stage, _, i_cur in pairs:
        if stage != at_stage:
            at_stage, before = stage, set()
        motion[i_cur] = before | {f"{i_cur}_mv.bin"}
        before = motion[i_cur]
    # decode_gop: the last stage first; both results of a pair depend on both of its entries and on its motion
    by_stage = {}
    for stage, i_ref, i_cur in pairs:
        by_stage.setdefault(stage, []).append((i_ref, i_cur))
    for stage in sorted(by_stage, reverse=True):
        for i_ref, i_cur in reversed(by_stage[stage]):
            both = entry[i_ref] | entry[i_cur] | motion[i_cur]
            entry[i_ref], entry[i_cur] = both, set(both)
    need = set().union(*(entry[t] for t in wanted))
    return [n for n in all_files(size) if n in need]
