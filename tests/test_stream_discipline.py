"""Source-level stream discipline of the HIP sources (zk-odst_amd/csrc/*.hip, *.h).

include/b2f.h promises that every `*_dev` call is stream-ordered on the caller's stream. Two
properties keep that promise and are cheap to read off the text:

  1  every hipLaunchKernelGGL passes a stream expression as its launch stream (the fifth macro
     argument, after kernel, grid, block and LDS bytes), never a literal 0 / nullptr (the two
     diagnostics probes, which have no stream argument and block end to end, are listed);
  2  every blocking-form hipMemset / hipMemcpy / hipMemcpyToSymbol / hipMemcpyFromSymbol -- a
     null-stream operation a caller's non-blocking stream is not ordered against -- sits in a
     function of the allowlist below, each entry with its reason.

tests/test_gpu_side_stream.py runs the calls on a non-blocking stream behind in-flight work; this
module keeps a new launch or copy from leaving the stream without anyone running anything."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zk-odst_amd", "csrc")

# (file, function) -> (reason, macro the site must be compiled under, or None)
ALLOWED = {
    ("b2f_kernels.hip", "b2f_create"):
        ("zeroes the status block before any call exists; the host waits for the clear", None),
    ("b2f_kernels.hip", "ensure_clock"):
        ("diagnostics clock block, zeroed when first allocated (EVAL_CLOCK variants only)", None),
    ("b2f_kernels.hip", "b2f_debug_clock"):
        ("diagnostics read-out after hipDeviceSynchronize", None),
    ("b2f_kernels.hip", "b2f_debug_eval_path"):
        ("test hook, reads one word after hipDeviceSynchronize", None),
    ("b2f_kernels.hip", "b2f_sync"):
        ("reads the sticky word after synchronizing the caller's stream", None),
    ("b2f_kernels.hip", "b2f_fill"):
        ("host-pointer convenience: documented as blocking", None),
    ("b2f_kernels.hip", "b2f_eval"):
        ("host-pointer convenience: documented as blocking", None),
    ("b2f_api_prover.hip", "perm_patterns"):
        ("pattern pool rebuilt for a new `rounds`: blocking copy after a stream synchronize", None),
    ("b2f_lookup.hip", "run_lookup"):
        ("the corrupt-a-cell switch of the diagnostics build", "B2F_DIAG"),
    ("b2f_lookup.hip", "b2f_debug_lk_clock"):
        ("phase-clock read-out of a profiling variant", "B2F_LK_CLOCK"),
    ("b2f_fieldprobe.hip", "field_op"):
        ("field primitive probe: host arrays in, host arrays out, blocking", None),
    ("b2f_curveprobe.hip", "curve_op"):
        ("curve operation probe: host arrays in, host arrays out, blocking", None),
}

# (file, function) -> reason: the only launches that may name the null stream. Both probes take host
# arrays and no stream, and launch between their own blocking copies and a hipDeviceSynchronize.
NULL_STREAM_LAUNCH = {
    ("b2f_fieldprobe.hip", "field_op"): "diagnostics probe without a stream argument, blocking end to end",
    ("b2f_curveprobe.hip", "curve_op"): "diagnostics probe without a stream argument, blocking end to end",
}

BLOCKING = re.compile(r"\b(hipMemset|hipMemcpy|hipMemcpyToSymbol|hipMemcpyFromSymbol)\s*\(")
LAUNCH = re.compile(r"\bhipLaunchKernelGGL\s*\(")
NULL_STREAM = re.compile(r"^(\(\s*hipStream_t\s*\))?\s*\(?\s*(0|nullptr|NULL|hipStreamDefault|hipStreamLegacy)\s*\)?$")
NOT_A_FUNCTION = {"__attribute__", "visibility", "__launch_bounds__", "defined", "if", "for", "while", "switch"}


def strip_comments_and_strings(text):
    """Comments and the contents of string / character literals replaced by spaces, newlines kept,
    so offsets and line numbers are those of the file."""
    out, i, n = [], 0, len(text)
    while i < n:
        two = text[i:i + 2]
        if two == "//":
            j = text.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i))
            i = j
        elif two == "/*":
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("".join(c if c == "\n" else " " for c in text[i:j]))
            i = j
        elif text[i] in "\"'":
            q, j = text[i], i + 1
            while j < n and text[j] != q and text[j] != "\n":
                j += 2 if text[j] == "\\" else 1
            j = min(j + 1, n)
            out.append(q + " " * (j - i - 2) + q if j - i >= 2 else text[i:j])
            i = j
        else:
            out.append(text[i])
            i += 1
    return "".join(out)


def call_arguments(text, open_paren):
    """The top-level arguments of the call whose '(' is at text[open_paren]; commas inside (), [] and
    {} do not split (a kernel name with template commas is parenthesised: the launch is a macro)."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        c = text[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i])
                return [" ".join(a.replace("\\\n", " ").split()) for a in args]
        elif c == "," and depth == 1:
            args.append(text[start:i])
            start = i + 1
    raise AssertionError("unbalanced call")


def enclosing_function(lines, line_no):
    """Name of the function a (1-based) line belongs to: function headers start in column 0 in
    these sources, bodies are indented."""
    for i in range(line_no - 1, -1, -1):
        ln = lines[i]
        if not ln or ln[0] in " \t}#" or "(" not in ln:
            continue
        names = [m for m in re.findall(r"\b([A-Za-z_]\w*)\s*\(", ln) if m not in NOT_A_FUNCTION]
        if names:
            return names[0]
    return None


def macros_around(lines, line_no):
    """The #if / #ifdef conditions open at a (1-based) line, #else branches marked with '!'."""
    stack = []
    for ln in lines[:line_no - 1]:
        m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif|else|endif)\b\s*(.*)", ln)
        if not m:
            continue
        kind, cond = m.group(1), m.group(2).strip()
        if kind in ("ifdef", "if"):
            stack.append(cond)
        elif kind == "ifndef":
            stack.append("!" + cond)
        elif kind in ("else", "elif"):
            stack[-1] = "!" + stack[-1]
        elif stack:
            stack.pop()
    return stack


def violations(name, raw):
    """(line, message) for every launch on a literal null stream and every blocking copy or memset
    outside the allowlist in one source text."""
    text = strip_comments_and_strings(raw)
    lines = text.split("\n")
    found = []
    for m in LAUNCH.finditer(text):
        line_no = text.count("\n", 0, m.start()) + 1
        args = call_arguments(text, m.end() - 1)
        if len(args) < 5:
            found.append((line_no, "hipLaunchKernelGGL with %d arguments: no stream" % len(args)))
        elif (NULL_STREAM.match(args[4]) or not args[4]) \
                and (name, enclosing_function(lines, line_no)) not in NULL_STREAM_LAUNCH:
            found.append((line_no, "hipLaunchKernelGGL on the null stream (%r)" % args[4]))
    for m in BLOCKING.finditer(text):
        line_no = text.count("\n", 0, m.start()) + 1
        fn = enclosing_function(lines, line_no)
        entry = ALLOWED.get((name, fn))
        if entry is None:
            found.append((line_no, "blocking %s in %s(): not on the allowlist" % (m.group(1), fn)))
        elif entry[1] is not None and entry[1] not in macros_around(lines, line_no):
            found.append((line_no, "blocking %s in %s(): allowed only under #ifdef %s" % (m.group(1), fn, entry[1])))
    return found


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(paths) >= 20, "the HIP sources moved: %s" % CSRC
    for path in paths:
        with open(path) as fh:
            yield os.path.basename(path), fh.read()


def test_every_launch_names_a_stream_and_blocking_copies_are_listed():
    bad, launches, blocking, used = [], 0, 0, set()
    for name, raw in _sources():
        text = strip_comments_and_strings(raw)
        launches += len(LAUNCH.findall(text))
        lines = text.split("\n")
        for m in BLOCKING.finditer(text):
            blocking += 1
            used.add((name, enclosing_function(lines, text.count("\n", 0, m.start()) + 1)))
        bad += ["%s:%d: %s" % (name, line, msg) for line, msg in violations(name, raw)]
    assert not bad, "\n".join(bad)
    # the scan saw the sources it is meant to see, and the allowlist holds no dead entry
    assert launches >= 80 and blocking >= 30, (launches, blocking)
    assert used == set(ALLOWED), sorted(set(ALLOWED) ^ used)


def test_the_scan_flags_what_it_should():
    """The checker on a text with one fault of each kind (and their accepted twins)."""
    src = '''
namespace {
int helper(b2f_ctx* ctx, hipStream_t s) {
  hipLaunchKernelGGL(kern<F>, dim3(g, 2), dim3(256), 0, s, a, b);            // fine
  hipLaunchKernelGGL((kern2<F, true>), dim3(g), dim3(256), 0, 0, a, b);      // null stream
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), 0, (hipStream_t)nullptr, a);  // null stream
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), 0, side.s2 ? side.s2 : s, a); // fine
  // hipMemset(p, 0, n) in a comment, "hipMemcpy(" in a string: neither counts
  const char* msg = "hipMemcpy(x)";
  hipMemsetAsync(p, 0, n, s);
  hipMemcpyAsync(p, q, n, hipMemcpyHostToDevice, s);
  return hipMemset(p, 0, n);                                                 // not listed
}
}  // namespace
B2F_API int b2f_sync(b2f_ctx* ctx,
                     void* stream) {
  HIPCHK(ctx, hipMemcpy(&bits, ctx->d_status + 2, sizeof bits, hipMemcpyDeviceToHost));
  return 0;
}
hipError_t run_lookup(int x) {
#ifdef B2F_DIAG
  hipMemcpyToSymbol(HIP_SYMBOL(g), &x, 4);
#else
  hipMemcpyToSymbol(HIP_SYMBOL(g), &x, 4);                                   // product build
#endif
  return hipSuccess;
}
'''
    got = violations("b2f_kernels.hip", src)
    assert [line for line, _ in got] == [5, 6, 12, 22, 24], got  # b2f_sync is listed for this file
    assert "helper()" in got[2][1] and "run_lookup()" in got[3][1]
    got = violations("b2f_lookup.hip", src)
    assert [line for line, _ in got] == [5, 6, 12, 17, 24], got  # run_lookup is, under B2F_DIAG only
    assert "b2f_sync()" in got[3][1] and "B2F_DIAG" in got[4][1]
