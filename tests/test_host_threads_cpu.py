"""The inventory behind tests/test_gpu_host_threads.py, without a GPU: every dict cache of HipEngine is filled
under _cache_lock or listed with the reason it needs none; every thread_local, std::once_flag, function-static initialiser
and file-scope mutable of csrc/ is listed with its kind; every stream and event attribute of the engine is listed with the
threaded case that reaches it; and the rows the four threads of the C-ABI test walk are rows of the censuses that run at
the default knobs.  Something added later without a line in tests/host_threads.py fails here."""
import ast
import glob
import os
import re

import host_threads as ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = os.path.join(ROOT, "learned-pmctf_amd", "pMCTF", "hip", "engine.py")
CSRC = os.path.join(ROOT, "learned-pmctf_amd", "csrc")


def _engine_class(text=None):
    tree = ast.parse(text if text is not None else open(ENGINE).read())
    return next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "HipEngine")


def _self_attr(node):
    return node.attr if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "self" \
        else None


def engine_caches(text=None):
    """names of the attributes HipEngine.__init__ binds to a dict: a literal (empty or not) or dict(...)"""
    init = next(n for n in _engine_class(text).body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    out = []
    for n in ast.walk(init):
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and _self_attr(n.targets[0]):
            v = n.value
            if isinstance(v, ast.Dict) or (isinstance(v, ast.Call) and getattr(v.func, "id", "") in ("dict", "OrderedDict")):
                out.append(_self_attr(n.targets[0]))
    return out


def stores_under_lock(method, cache, text=None):
    """(stores into self.<cache>[...] inside `with self._cache_lock`, stores outside it) within HipEngine.<method>"""
    fn = next(n for n in _engine_class(text).body if isinstance(n, ast.FunctionDef) and n.name == method)
    inside, outside = 0, 0

    def visit(node, locked):
        nonlocal inside, outside
        if isinstance(node, ast.With):
            locked = locked or any(_self_attr(i.context_expr) == "_cache_lock" for i in node.items)
        if isinstance(node, ast.Assign):
            for t in node.targets:
                if isinstance(t, ast.Subscript) and _self_attr(t.value) == cache:
                    inside, outside = inside + locked, outside + (not locked)
        for ch in ast.iter_child_nodes(node):
            visit(ch, locked)
    visit(fn, False)
    return inside, outside


def test_every_dict_cache_of_the_engine_is_locked_or_classified():
    found = engine_caches()
    assert sorted(found) == sorted(ht.ENGINE_CACHES), (sorted(set(found) ^ set(ht.ENGINE_CACHES)))
    for name, (kind, what) in ht.ENGINE_CACHES.items():
        assert kind in ("locked", "per-thread", "host-only") and what
        if kind == "locked":
            assert stores_under_lock(what, name) == (1, 0), f"{name}: HipEngine.{what} must fill it under _cache_lock only"
    text = open(ENGINE).read()
    # nothing else of the engine stores into a locked cache
    for name, (kind, what) in ht.ENGINE_CACHES.items():
        if kind == "locked":
            assert len(re.findall(rf"self\.{name}\[[^\]]*\]\s*=[^=]", text)) == 1, name


def test_the_cache_scan_sees_a_new_cache_and_a_fill_outside_the_lock():
    text = open(ENGINE).read()
    more = text.replace("        self._convs = {}\n", "        self._convs = {}\n        self._new_cache = {}\n", 1)
    assert more != text and "_new_cache" in engine_caches(more)
    unlocked = ("class HipEngine:\n    def conv(self, key):\n        c = self._convs.get(key)\n        if c is None:\n"
                "            c = self._convs[key] = 1\n        return c\n")
    assert stores_under_lock("conv", "_convs", unlocked) == (0, 1)


# ------------------------------------------------------------------------------------------------------------ the csrc
def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


_NOT_A_TYPE = ("return", "using", "typedef", "template", "namespace", "struct", "class", "enum", "extern", "if", "else",
               "case", "goto", "const", "constexpr", "inline", "static", "__global__", "__device__", "__constant__",
               "__shared__", "__host__", "__forceinline__")


def c_state(texts=None):
    """{(file, name): kind} read from csrc/*.hip and csrc/*.h: thread_local objects, std::once_flag objects (function
    parameters aside), function-static objects with an initialiser, and file-scope objects that are neither const nor
    constexpr nor device memory (those are the process-wide mutables)"""
    out = {}
    if texts is None:
        texts = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*")))
                 if p.endswith((".hip", ".h"))}
    for name, text in texts.items():
        text = _strip_comments(text)
        text = re.sub(r"^[ \t]*#.*?(?<!\\)$", "", text, flags=re.M | re.S)              # preprocessor lines, continued ones too
        for m in re.finditer(r"\bthread_local\b[^;=(]*?\b(\w+)\s*(?:\[[^\]]*\])?\s*(?:=[^;]*)?;", text):
            out[(name, m.group(1))] = "thread_local"
        for m in re.finditer(r"\bstd::once_flag\s+(?!&)([\w\[\], ]+);", text):
            for v in m.group(1).split(","):
                out[(name, re.sub(r"\[.*", "", v).strip())] = "once_flag"
        for m in re.finditer(r"^[ \t]+static\s+(?!std::once_flag\b)(?!__device__|__constant__|constexpr\b)([^;(]*?)\b(\w+)\s*"
                             r"(?:\[[^\]]*\])*\s*=", text, flags=re.M):
            out.setdefault((name, m.group(2)), "function-static")
        # file scope: a declaration that starts in column 0, `type name[..] [= ...];` or `type name[] = {`
        for m in re.finditer(r"^(?:static\s+)?((?:[\w:]+(?:<[^;>]*>)?[\s\*&]+)+)(\w+)\s*(?:\[[^\]]*\])*\s*(?:=|;)", text,
                             flags=re.M):
            words = m.group(1).split()
            line = text[m.start():text.index("\n", m.start())]
            if words[0] in _NOT_A_TYPE or "thread_local" in words or "(" in m.group(1) or words[0] == "std::once_flag" \
                    or re.match(r"(static\s+)?(const|constexpr|__device__|__constant__|inline|extern)\b", line):
                continue
            out.setdefault((name, m.group(2)), "process-wide")
    return out


def test_every_per_thread_and_process_wide_object_of_csrc_is_classified():
    found = c_state()
    assert found == ht.C_STATE, {k: (found.get(k), ht.C_STATE.get(k)) for k in set(found) | set(ht.C_STATE)
                                 if found.get(k) != ht.C_STATE.get(k)}
    kinds = set(found.values())
    assert kinds >= {"thread_local", "once_flag", "process-wide"}
    # the per-thread records and the summation rule are what the threads of part 1 differ in: all five are thread_local
    assert sum(1 for v in found.values() if v == "thread_local") == 5
    assert sum(1 for v in found.values() if v == "once_flag") >= 17


def test_the_csrc_scan_sees_what_is_added():
    src = ("namespace {\nthread_local int t_new = 0;\nint g_counter = 0;\nstatic float g_table[4] = {0};\n"
           "const int fixed = 3;\nconstexpr int also_fixed = 4;\nstatic __device__ const int dev[2] = {1, 2};\n"
           "int f(int a) {\n    static std::once_flag once_new, once_more[4];\n    static const bool on = getenv(\"X\") != 0;\n"
           "    int local = 0;\n    return a;\n}\nvoid g(std::once_flag &flag);\n}\n")
    assert c_state({"x.hip": src}) == {("x.hip", "t_new"): "thread_local", ("x.hip", "g_counter"): "process-wide",
                                       ("x.hip", "g_table"): "process-wide", ("x.hip", "once_new"): "once_flag",
                                       ("x.hip", "once_more"): "once_flag", ("x.hip", "on"): "function-static"}


# ------------------------------------------------------------------------------------------------- streams and events
def engine_streams(text=None):
    """every attribute of HipEngine bound anywhere in the class whose name says stream or event, and every attribute
    bound to (or extended by) a torch.cuda.Stream / torch.cuda.Event"""
    cls = _engine_class(text)
    out = set()

    def makes_stream(v):
        return any(isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr in ("Stream", "Event")
                   for c in ast.walk(v))
    for n in ast.walk(cls):
        if isinstance(n, ast.Assign):
            targets = [e for t in n.targets for e in (t.elts if isinstance(t, ast.Tuple) else [t])]
            for t in targets:
                base = t.value if isinstance(t, ast.Subscript) else t
                a = _self_attr(base)
                if a and (re.search(r"stream|event", a) or makes_stream(n.value)):
                    out.add(a)
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "append" \
                and _self_attr(n.func.value) and n.args and makes_stream(n.args[0]):
            out.add(_self_attr(n.func.value))
    return out


def test_every_stream_and_event_of_the_engine_names_the_case_that_reaches_it():
    found = engine_streams()
    assert found == set(ht.ENGINE_STREAMS), found ^ set(ht.ENGINE_STREAMS)
    for name, (what, cases) in ht.ENGINE_STREAMS.items():
        assert what and all(c in ht.CASES for c in cases), (name, cases)
        assert cases or "not a stream" in what, f"{name}: a stream that no threaded case reaches"
    more = open(ENGINE).read().replace("        self.batch_streams = []",
                                       "        self.batch_streams = []\n        self.copy_stream = torch.cuda.Stream()", 1)
    assert "copy_stream" in engine_streams(more)
    # every case exists in the child runner and in the GPU test's groups
    child = open(os.path.join(ROOT, "tests", "host_threads_child.py")).read()
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_host_threads.py")).read()
    for case in ht.CASES:
        assert f"def case_{case}(" in child and f'"{case}"' in gpu, case


# --------------------------------------------------------------------------------------------- the rows of the C-ABI test
def test_the_rows_of_the_four_threads_are_census_rows_that_run_at_the_default_knobs():
    import conv_census as cc
    import ew_census as ec
    import valu_conv_census as vc
    assert len(ht.ROWS) == 4
    seen = set()
    for rows in ht.ROWS:
        assert {r[0] for r in rows} == {"conv", "valu", "ew"}
        for r in rows:
            assert (r[0], r[1]) not in seen, f"{r}: the threads' lists are disjoint"
            seen.add((r[0], r[1]))
            if r[0] == "conv":
                row = cc.row(r[1])
                assert row[6] == ht.CONV_KNOBS_BY_OPTS[r[1]], (r, row[6])
                opts = r[2] if len(r) > 2 else None
                if row[6].get("MSPLIT_PX") == 0:
                    assert opts == ht.NO_MSPLIT and row[6].get("NT", 1) == 1 and row[7][0][1] >= 7 and row[1][6] == 1
                    N, Cin, H, W, Cout, K, S, pad = row[1]
                    assert N * cc.out_hw(row[1])[0] * cc.out_hw(row[1])[1] < cc.KNOBS["BIGPX"]
                else:
                    assert opts is None
                    px = row[1][0] * cc.out_hw(row[1])[0] * cc.out_hw(row[1])[1]
                    assert not row[6] or (set(row[6]) == {"MSPLIT_PX"} and px <= cc.KNOBS["MSPLIT_PX"])
            elif r[0] == "valu":
                assert vc.row(r[1])[8] is None, f"{r}: a row behind an environment switch"
            else:
                row = ec.row(r[1])
                assert all(op in ec.ops_of(row) for op in ht.EW_OPS)
    conv = [cc.row(r[1]) for rows in ht.ROWS for r in rows if r[0] == "conv"]
    assert {c[2] for c in conv} == {0, 1, 32}, "rule chain, rule blocks and reduce-32 on the MFMA entry"
    with_opts = [r for rows in ht.ROWS for r in rows if r[0] == "conv" and len(r) > 2]
    assert 0 < len(with_opts) < len(conv)
    # one geometry and rule with and without launch options: two different kernels shapes from the same call
    a, b = cc.row("msplit_pipe33_mtp7_chain"), cc.row("pipe33_chain_mt7")
    assert a[1] == b[1] and a[2] == b[2] and a[7] != b[7]
    valu = [vc.row(r[1]) for rows in ht.ROWS for r in rows if r[0] == "valu"]
    assert {v[3] for v in valu} >= {1, 2, 3} and {v[1] for v in valu} >= {"smallcin", "cin1_dual"}
    ew = {ec.row(r[1])[6] for rows in ht.ROWS for r in rows if r[0] == "ew"}
    assert ew == {ec.FLAT_V, ec.C4_CH, ec.GEN_C, ec.C4_ROWS}
    assert 0 <= ht.REFUSED_THREAD < 4 and 4 <= ht.ROUNDS <= 64


def test_the_thread_runner_reports_errors_and_overlap():
    assert ht.pairwise_overlap([(0, 3), (1, 4), (2, 5)]) and not ht.pairwise_overlap([(0, 1), (0.5, 3), (2, 4)])
    assert ht.run_threads([lambda i=i: i * i for i in range(4)]) == [0, 1, 4, 9]
    crew = ht.Crew(2)
    import threading
    first = crew.run([threading.get_ident, threading.get_ident])
    assert crew.run([threading.get_ident, threading.get_ident]) == first and len(set(first)) == 2, "the threads stay"

    def boom():
        raise ValueError("x")
    try:
        crew.run([boom, lambda: 1])
    except AssertionError as e:
        assert "host thread 0: ValueError" in str(e)
    else:
        raise AssertionError("an error on a thread must surface")
    crew.close()
    assert not crew.stuck
