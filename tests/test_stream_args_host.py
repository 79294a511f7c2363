"""The stream arguments of the library's own sources, read as text (CPU; no GPU, no compiler).

tests/test_gpu_streams.py runs the device API on a caller's stream and sees a launch on the wrong stream where it writes a caller's buffer.  A launch
on the null stream that only writes library-owned scratch, and a blocking runtime call in a path documented as asynchronous, it cannot see: this
file can.  Over cholesky_amd/csrc/*.hip, *.cpp and *.h (comments and string literals blanked):

  * every hipLaunchKernelGGL(, hip*Async( and hipEventRecord( call is joined up to its closing parenthesis and its stream argument (the fifth of a
    launch, the last of the others) must be an expression: not the literal 0, nullptr, NULL or a cast of one;
  * the blocking hipMemcpy(, hipMemset(, hipMemcpy2D( and hipDeviceSynchronize( may appear only in the (file, function) pairs of BLOCKING_ALLOWED,
    each with the reason it may block there, and every pair of the list must still hold such a call (a stale entry fails).  hipStreamSynchronize(st) is not in the
    list: it names its stream, and a call that uses it in a warm asynchronous path is refused by the capture test of tests/test_gpu_streams.py.

The enclosing function is the last line at brace depth 0 that starts a definition (the name before its first parenthesis; a struct's methods go by
the struct's name)."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cholesky_amd", "csrc")

ENQUEUE = re.compile(r"\b(hipLaunchKernelGGL|hip\w*Async|hipEventRecord)\s*\(")
BLOCKING = re.compile(r"\b(hipMemcpy|hipMemset|hipMemcpy2D|hipDeviceSynchronize)\s*\(")
NOT_CODE = re.compile(r"""//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|'(?:\\.|[^'\\\n])*'""", re.S)
NULL_STREAM = re.compile(r"^(\(\s*hipStream_t\s*\)\s*)?\(?\s*(0|nullptr|NULL)\s*\)?$")

# (file, function): why a blocking runtime call is right there.  Everything else in the library enqueues on the caller's stream.
BLOCKING_ALLOWED = {
    ("chol_api.cpp", "poison_fill"): "CHOLAMD_POISON: the NaN fill of a fresh allocation, ordered before work on any stream",
    ("chol_api.cpp", "chol_dev_zero"): "dev_buf::alloc_zero at creation and first use: cleared on the null stream, then the device is synchronised",
    ("chol_api.cpp", "chol_dev_copy_in"): "dev_buf::upload at creation and first use: a blocking copy from pageable host memory",
    ("chol_api.cpp", "cholamd_device_destroy"): "destroy waits for the work in flight before it frees",
    ("chol_api.cpp", "cholamd_device_free_arena"): "a rank arena is unmapped only when the device is idle",
    ("chol_api_factor.cpp", "cholamd_device_program_trace"): "diagnostic: reads the job stamps back after synchronising the stream",
    ("chol_api_factor.cpp", "cholamd_factor_info"): "documented: called after the stream has been synchronised, reads two ints back",
    ("chol_api.cpp", "f32_range_ok"): "the fp32 range verdict's refusal: the offending value read back for the error text, on the way to CHOLAMD_ERR_ARG",
    ("chol_api_blas.cpp", "debug_dump"): "cholamd_factor_debug: the arena read back for the dump files",
    ("chol_api_blas.cpp", "cholamd_factor_debug"): "cholamd_factor_debug: a failed pivot's info written where cholamd_factor_info reads it",
    ("chol_api_blas.cpp", "cholamd_dpotrf_dev"): "per-call BLAS wrapper: run_potrf has synchronised and read info back; info written to the caller's device word",
    ("chol_api_blas.cpp", "host_mat"): "per-call BLAS host wrappers (host pointers): copy in, run, copy back",
    ("chol_api_blas.cpp", "cholamd_cblas_dgemv"): "per-call BLAS host wrapper (host pointers): copy in, run, copy back",
}


def blank(text):
    """`text` with comments, string and character literals replaced by spaces of the same length (newlines kept)."""
    return NOT_CODE.sub(lambda m: re.sub(r"[^\n]", " ", m.group(0)), text)


def call_args(code, open_paren):
    """The top-level arguments of the call whose opening parenthesis is at `open_paren`, and the index after its closing one."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(code)):
        c = code[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(code[start:i])
                return [" ".join(a.split()) for a in args], i + 1
        elif c == "," and depth == 1:
            args.append(code[start:i])
            start = i + 1
    raise AssertionError("unbalanced call")


def function_starts(code):
    """[(offset, name)] of the definitions at brace depth 0, in order; asserts that the braces of the file balance."""
    out, depth, pos = [], 0, 0
    for line in code.split("\n"):
        if depth == 0 and re.match(r"[A-Za-z_]", line):
            head = line.split("(")[0] if "(" in line else line.split("{")[0]
            names = re.findall(r"[A-Za-z_]\w*", head)
            if names:
                out.append((pos, names[-1]))
        if not line.startswith("#"):
            depth += line.count("{") - line.count("}")
        assert depth >= 0, (line, pos)
        pos += len(line) + 1
    assert depth == 0, "unbalanced braces"
    return out


def enclosing(starts, offset):
    name = None
    for pos, nm in starts:
        if pos > offset:
            break
        name = nm
    return name


def scan(files):
    """(enqueueing calls as (file, line, function, call name, stream argument), blocking calls as (file, line, function, call name))."""
    enq, blk = [], []
    for path in files:
        with open(path) as f:
            code = blank(f.read())
        starts = function_starts(code)
        fn = os.path.basename(path)
        for m in ENQUEUE.finditer(code):
            if code[:m.start()].rstrip().endswith("#define"):
                continue
            args, _ = call_args(code, m.end() - 1)
            line = code.count("\n", 0, m.start()) + 1
            launch = m.group(1) == "hipLaunchKernelGGL"
            assert len(args) >= (5 if launch else 2), (fn, line, args)
            enq.append((fn, line, enclosing(starts, m.start()), m.group(1), args[4] if launch else args[-1]))
        for m in BLOCKING.finditer(code):
            blk.append((fn, code.count("\n", 0, m.start()) + 1, enclosing(starts, m.start()), m.group(1)))
    return enq, blk


def sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) >= 20
    return files


@pytest.fixture(scope="module")
def scanned():
    return scan(sources())


def null_stream_calls(enq):
    return [e for e in enq if NULL_STREAM.match(e[4])]


def test_the_scanner_sees_the_calls(scanned):
    """Every kernel family's launcher file and the glue are read: well over a hundred launches, the asynchronous copies and the timers' events."""
    enq, blk = scanned
    by_kind = {}
    for e in enq:
        by_kind[e[3]] = by_kind.get(e[3], 0) + 1
    assert by_kind.get("hipLaunchKernelGGL", 0) >= 100 and by_kind.get("hipMemcpyAsync", 0) >= 10 and by_kind.get("hipEventRecord", 0) >= 4, by_kind
    files = {e[0] for e in enq}
    for fn in ("chol_kernels.hip", "chol_solve.hip", "chol_kernels_f32.hip", "chol_solve_nrhs.hip", "chol_solve_det.hip", "chol_pcg.hip", "chol_selinv.hip",
               "chol_multiply.hip", "chol_api.cpp", "chol_api_factor.cpp", "chol_api_solve.cpp", "chol_api_query.cpp", "chol_api_pcg.cpp", "chol_api_schur.cpp",
               "chol_api_blas.cpp", "chol_api_lowrank.cpp", "chol_device.h"):
        assert fn in files, fn
    assert all(e[2] for e in enq) and all(b[2] for b in blk)


def test_every_enqueue_names_a_stream(scanned):
    bad = null_stream_calls(scanned[0])
    assert not bad, "launches, asynchronous copies or event records on the null stream:\n" + "\n".join(f"  {f}:{ln} {fn}: {c}(..., {a})" for f, ln, fn, c, a in bad)


def test_blocking_calls_only_where_listed(scanned):
    found = {}
    for f, ln, fn, c in scanned[1]:
        found.setdefault((f, fn), []).append(f"{f}:{ln} {c}")
    extra = {k: v for k, v in found.items() if k not in BLOCKING_ALLOWED}
    assert not extra, f"blocking runtime calls outside BLOCKING_ALLOWED: {extra}"
    stale = [k for k in BLOCKING_ALLOWED if k not in found]
    assert not stale, f"BLOCKING_ALLOWED lists functions without a blocking call: {stale}"
    assert all(len(reason) > 10 for reason in BLOCKING_ALLOWED.values())


SAMPLE = """
// hipLaunchKernelGGL(k_comment, dim3(1), dim3(1), 0, 0);
static int launch_good(int n, hipStream_t st)
{
  hipLaunchKernelGGL((k_two<double, 1>), dim3(n, (n + 1) / 2), dim3(256), 0, st, n,
                     "0, 0);");
  return 0;
}
template <class T> int launch_bad(int n, hipStream_t st)
{
  if (n) { hipLaunchKernelGGL(k_one<T>, dim3(n), dim3(64),
                              0, 0, n); }
  HIPCHK(hipMemcpyAsync(a, b, n, hipMemcpyDeviceToDevice, nullptr));
  HIPCHK(hipMemsetAsync(a, 0, n, (hipStream_t)0));
  (void)hipEventRecord(ev, NULL);
  (void)hipEventRecord(ev, streams ? (hipStream_t)streams[0] : nullptr);
  return 0;
}
struct holder {
  int pull() { return hipMemcpy(h, d, 8, hipMemcpyDeviceToHost) != hipSuccess; }
};
"""


def test_the_scanner_on_a_sample(tmp_path):
    """The rules on a text with known answers: a comment and a string are not code, a parenthesised template name is one argument, a call may span
    lines, every spelling of the null stream is found, a conditional that names a stream is an expression, and calls are attributed to their function."""
    p = tmp_path / "sample.cpp"
    p.write_text(SAMPLE)
    enq, blk = scan([str(p)])
    assert [(e[2], e[3], e[4]) for e in enq] == [
        ("launch_good", "hipLaunchKernelGGL", "st"), ("launch_bad", "hipLaunchKernelGGL", "0"), ("launch_bad", "hipMemcpyAsync", "nullptr"),
        ("launch_bad", "hipMemsetAsync", "(hipStream_t)0"), ("launch_bad", "hipEventRecord", "NULL"),
        ("launch_bad", "hipEventRecord", "streams ? (hipStream_t)streams[0] : nullptr")]
    assert [(e[2], e[4]) for e in null_stream_calls(enq)] == [("launch_bad", "0"), ("launch_bad", "nullptr"), ("launch_bad", "(hipStream_t)0"), ("launch_bad", "NULL")]
    assert [(b[2], b[3], b[1]) for b in blk] == [("holder", "hipMemcpy", 20)]


def test_a_launcher_with_its_stream_turned_into_zero_is_found(tmp_path):
    """Every launcher of every .hip file in turn: its `st` replaced by 0 in a copy of the file, and the copy must fail the rule."""
    launchers = 0
    for path in sources():
        if not path.endswith(".hip"):
            continue
        with open(path) as f:
            text = f.read()
        code = blank(text)
        copy = tmp_path / os.path.basename(path)
        for m in re.finditer(r"\bhipLaunchKernelGGL\s*\(", code):
            args, end = call_args(code, m.end() - 1)
            assert args[4] == "st", (path, args[4])
            at = m.end() + re.search(r",\s*st\s*,", code[m.end():end]).start()     # (a kernel argument is never the bare `st`: it comes fifth)
            k = text.index("st", at)
            copy.write_text(text[:k] + "0" + text[k + 2:])
            bad = null_stream_calls(scan([str(copy)])[0])
            assert len(bad) == 1 and bad[0][1] == code.count("\n", 0, m.start()) + 1, (path, bad)
            launchers += 1
    assert launchers >= 90
