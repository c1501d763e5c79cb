"""The inventory behind tests/test_gpu_stream_order.py, without a GPU: every export of include/pmctf_hip.h that takes a
stream has a row in stream_order.ROWS (the others an exemption with its reason), every wrapper hands its entry the
current stream, and every launch and asynchronous runtime call of csrc/ names the stream it was given."""
import ast
import glob
import os
import re

import stream_order as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pmctf_hip.h")
HIP_PY = os.path.join(ROOT, "learned-pmctf_amd", "pMCTF", "hip")
CSRC = os.path.join(ROOT, "learned-pmctf_amd", "csrc")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def exports():
    """name -> parameter text of every function prototype of the header"""
    text = _strip_comments(open(HEADER).read())
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(pmctf_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        assert m.group(1) not in out, m.group(1)
        out[m.group(1)] = " ".join(m.group(2).split())
    return out


def stream_takers():
    return {n for n, params in exports().items() if re.search(r"\bvoid \*stream$", params)}


def test_the_header_parses_into_the_library_s_exports():
    """the parse is the whole ABI: the same names as the ctypes signatures of pMCTF/hip/lib.py, which the loader checks
    against the built library"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "learned-pmctf_amd"))
    text = open(os.path.join(HIP_PY, "lib.py")).read()
    sigs = set(re.findall(r'^    "(pmctf_\w+)":', text[:text.index("_RANS_SIGS")], flags=re.M))
    assert set(exports()) == sigs
    assert all(("stream" in p) == p.endswith("void *stream") for p in exports().values()), "a stream that is not last"


def test_every_export_has_a_row_or_an_exemption():
    takers, rows, exempt = stream_takers(), {r.entry for r in so.ROWS}, set(so.EXEMPT)
    assert len(takers) == 62
    assert rows == takers, (sorted(takers - rows), sorted(rows - takers))
    assert not rows & exempt
    assert rows | exempt == set(exports()), sorted(set(exports()) - rows - exempt)
    assert all(isinstance(v, str) and v for v in so.EXEMPT.values())
    names = [r.name for r in so.ROWS]
    assert len(names) == len(set(names))


def test_the_launch_paths_of_the_multi_launch_entries_have_rows_of_their_own():
    per_entry = {}
    for r in so.ROWS:
        per_entry.setdefault(r.entry, []).append(r.name)
    need = {"pmctf_conv2d_nhwc_opts_f32": ("rounds+remainder", "4+3 tiles"), "pmctf_resize_yuv420_u8": ("x pass", "y pass"),
            "pmctf_convert_chroma_u8": ("444->422", "422->420"), "pmctf_frame_quality_f32": ("front end", "msssim"),
            "pmctf_ll_ar_decode_rules_f32": ("row2", "row", "stream", "v1"), "pmctf_ll_ar_decode_batch_f32": ("two planes",),
            "pmctf_luma_activity_f32": ("no prev",), "pmctf_frame_sse_u16_f32": ("clear",)}
    for entry, words in need.items():
        for w in words:
            assert any(n.endswith(w) for n in per_entry[entry]), (entry, w, per_entry[entry])


# ------------------------------------------------------------------------------------------------------- the wrappers
def _is_stream_expr(node):
    """_stream(), or <a named stream object>.cuda_stream wrapped in c_void_p: never None, never a number"""
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_stream" and not node.args:
        return True
    if isinstance(node, ast.Call) and getattr(node.func, "attr", getattr(node.func, "id", "")) == "c_void_p" \
            and len(node.args) == 1:
        a = node.args[0]
        return isinstance(a, ast.Attribute) and a.attr == "cuda_stream" and isinstance(a.value, (ast.Name, ast.Attribute))
    return False


def _entries_of(node):
    """the pmctf_* names an expression can evaluate to: L.pmctf_x, a conditional of such, getattr(L, f"pmctf_..._u8")"""
    names = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Attribute) and n.attr.startswith("pmctf_"):
            names.add(n.attr)
        if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "getattr" and len(n.args) == 2:
            pattern = "".join(v.value if isinstance(v, ast.Constant) else r"\w+" for v in n.args[1].values) \
                if isinstance(n.args[1], ast.JoinedStr) else None
            if pattern and pattern.startswith("pmctf_"):
                names |= {e for e in exports() if re.fullmatch(pattern, e)}
    return names


def wrapper_calls():
    """(file, line, entry names, last argument) of every call into the library from pMCTF/hip/*.py, calls through a local
    name bound to an entry (fn = L.pmctf_a if ... else L.pmctf_b; fn(...)) included"""
    out = []
    for path in sorted(glob.glob(os.path.join(HIP_PY, "*.py"))):
        tree = ast.parse(open(path).read())
        for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Module))]:
            bound = {}
            body = [n for n in ast.walk(fn)]
            for n in body:
                if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
                    names = _entries_of(n.value)
                    if names and not any(isinstance(c, ast.Call) and _entries_of(c.func) for c in ast.walk(n.value)
                                         if isinstance(c, ast.Call) and getattr(c.func, "id", "") != "getattr"):
                        bound[n.targets[0].id] = bound.get(n.targets[0].id, set()) | names
            for n in body:
                if not isinstance(n, ast.Call):
                    continue
                if isinstance(n.func, ast.Attribute) and n.func.attr.startswith("pmctf_"):
                    names = {n.func.attr}
                elif isinstance(n.func, ast.Name) and n.func.id in bound and isinstance(fn, ast.FunctionDef):
                    names = bound[n.func.id]
                else:
                    continue
                out.append((os.path.basename(path), n.lineno, names, n.args[-1] if n.args else None))
    return out


def test_every_wrapper_passes_the_current_stream_or_a_named_one():
    takers = stream_takers()
    seen, bad = set(), []
    for path, line, names, last in set((p, l, frozenset(n), a) for p, l, n, a in wrapper_calls()):
        if not names & takers:
            continue
        assert names <= takers, (path, line, names)
        seen |= names
        if last is None or not _is_stream_expr(last):
            bad.append(f"{path}:{line} {sorted(names)}: last argument {ast.dump(last) if last is not None else None}")
    assert not bad, "\n".join(bad)
    # the product calls all but the entries that only tests and the C ABI's users reach
    assert takers - seen == {"pmctf_conv2d_nhwc_f32", "pmctf_conv2d_nhwc_geom_f32", "pmctf_bilinear_up2_f32",
                             "pmctf_bilinear_down2_f32", "pmctf_lstm_gates_f32", "pmctf_ll_ar_decode_f32"}, takers - seen


def test_the_stream_check_refuses_what_it_must():
    ok = ["f(a, _stream())", "f(a, C.c_void_p(stream.cuda_stream))", "f(a, C.c_void_p(self.motion_stream.cuda_stream))"]
    no = ["f(a, None)", "f(a, 0)", "f(a, C.c_void_p(0))", "f(a, C.c_void_p(None))", "f(a, stream)", "f(a, _stream)",
          "f(a, C.c_void_p(torch.cuda.default_stream().cuda_stream))"]
    for src, want in [(s, True) for s in ok] + [(s, False) for s in no]:
        assert _is_stream_expr(ast.parse(src).body[0].value.args[-1]) == want, src


# ------------------------------------------------------------------------------------------------------------ the csrc
LAUNCHERS = {"hipLaunchKernelGGL": 4, "PM_LAUNCH": 4, "CONV_LAUNCH": 4}       # index of the stream argument
STREAMS = ("st", "(hipStream_t)stream", "stream")


def _args_at(text, i):
    """the top-level arguments of the call whose opening parenthesis is text[i]; a first argument that is a template-id
    without parentheses of its own (kernel<4, 8>) keeps its commas"""
    assert text[i] == "("
    depth, angle, args, cur, j = 0, 0, [], "", i
    while True:
        c = text[j]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return args, j
        if depth == 1 and not args and c == "<" and re.search(r"\w$", cur):
            angle += 1
        elif depth == 1 and not args and c == ">" and angle:
            angle -= 1
        if c == "," and depth == 1 and not angle:
            args.append(cur.strip())
            cur = ""
        elif j > i:
            cur += c
        j += 1


def launch_sites():
    """(file, line, macro, stream expression) of every launch and hip*Async call of csrc/, the launcher macros' own definitions aside"""
    out = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not path.endswith((".hip", ".h", ".cpp", ".hpp")):
            continue
        text = _strip_comments(open(path).read())
        text = text.replace("\\\n", " \n")                   # launches inside multi-line macros count like any other
        for m in re.finditer(r"\b(hipLaunchKernelGGL|PM_LAUNCH_NOTED|PM_LAUNCH|CONV_LAUNCH|hip\w+Async)\s*\(", text):
            args, _ = _args_at(text, m.end() - 1)
            name = m.group(1)
            if "__VA_ARGS__" in args or "..." in args:                       # the launcher macros' own definitions, checked by the test
                continue
            if name == "PM_LAUNCH_NOTED":                    # (kernel, [form,] grid, block, smem, stream, ...): two definitions
                k = 5 if os.path.basename(path) == "ew_ops.hip" else 4
            elif name in LAUNCHERS:
                k = LAUNCHERS[name]
            else:
                k = len(args) - 1                            # hipMemsetAsync, hipMemcpyAsync, ...: the stream is last
            out.append((os.path.basename(path), text.count("\n", 0, m.start()) + 1, name, args[k]))
    return out


def test_every_launch_and_async_call_of_csrc_names_its_stream():
    sites = launch_sites()
    assert len(sites) >= 102 and {s[2] for s in sites} >= {"PM_LAUNCH", "PM_LAUNCH_NOTED", "CONV_LAUNCH", "hipMemsetAsync"}
    bad = [s for s in sites if s[3] not in STREAMS]
    assert not bad, bad
    # `st` is the entry's stream argument and nothing else, wherever it is declared or handed on
    decl = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if path.endswith((".hip", ".h", ".cpp", ".hpp")):
            text = _strip_comments(open(path).read())
            decl += [(os.path.basename(path), m.group(1).strip()) for m in re.finditer(r"hipStream_t\s+st\s*=([^;]*);", text)]
            for m in re.finditer(r"\bhipStream_t\b(?!\s+st\b)(?!\))", text):
                raise AssertionError(f"{path}: a stream that is not called st: {text[m.start():m.start() + 60]!r}")
    assert len(decl) >= 12 and all(d == "(hipStream_t)stream" for _, d in decl), decl
    # the two macro definitions the sites go through hand the stream on unchanged
    launch_h = open(os.path.join(CSRC, "launch.h")).read()
    assert "hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__)" in launch_h
    conv = open(os.path.join(CSRC, "conv_mfma.hip")).read()
    assert "PM_LAUNCH(kernel, grid, block, smem, stream, __VA_ARGS__)" in conv


def test_the_launch_parser_reads_template_arguments_and_nested_calls():
    src = "PM_LAUNCH(k<4, 8>, dim3(g, 2), dim3(256), 0, (hipStream_t)stream, x, y);"
    assert _args_at(src, src.index("("))[0][:5] == ["k<4, 8>", "dim3(g, 2)", "dim3(256)", "0", "(hipStream_t)stream"]
    src = "CONV_LAUNCH((k<MT, 1, true>), grid, dim3(256), 2 * smem, st, b);"
    assert _args_at(src, src.index("("))[0][4] == "st"
    src = "hipMemsetAsync(p, 0, 3 * sizeof(uint64_t), 0)"
    assert _args_at(src, src.index("("))[0][-1] == "0"


# ----------------------------------------------------------------------------------------------------- hand-off sites
def handoff_sites():
    """{(file, function): {kind: count}} read from the source: attribute calls named like the kinds (torch.cuda.synchronize,
    a device-wide wait, is not a hand-off between two parties) and every call with non_blocking=True"""
    paths = sorted(glob.glob(os.path.join(HIP_PY, "*.py"))) + \
        [os.path.join(ROOT, "learned-pmctf_amd", "pMCTF", "models", "video", "pMCTF_L.py")]
    out = {}

    def visit(node, path, fn):
        for ch in ast.iter_child_nodes(node):
            inner = (fn + "." if fn else "") + ch.name if isinstance(ch, (ast.FunctionDef, ast.ClassDef)) else fn
            if isinstance(ch, ast.Call):
                kind = None
                if isinstance(ch.func, ast.Attribute) and ch.func.attr in so.SITE_KINDS:
                    v = ch.func.value
                    if not (ch.func.attr == "synchronize" and isinstance(v, ast.Attribute) and v.attr == "cuda"):
                        kind = ch.func.attr
                if any(k.arg == "non_blocking" and getattr(k.value, "value", None) is True for k in ch.keywords):
                    kind = "non_blocking"
                if kind:
                    d = out.setdefault((os.path.basename(path), fn), {})
                    d[kind] = d.get(kind, 0) + 1
            visit(ch, path, inner)
    for path in paths:
        visit(ast.parse(open(path).read()), path, "")
    return out


def test_the_site_table_is_the_source_s():
    found = handoff_sites()
    table = {(f, fn): counts for f, fn, counts, _, _ in so.SITES}
    assert len(table) == len(so.SITES)
    assert table == found, {k: (table.get(k), found.get(k)) for k in set(table) | set(found) if table.get(k) != found.get(k)}
    assert sum(sum(c.values()) for c in found.values()) >= 40
    for _, _, _, crosses, cases in so.SITES:
        assert crosses and cases and "unreached" not in cases
