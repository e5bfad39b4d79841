"""CPU: lstm_hip_score (include/lstm_hip.h) without a device -- the header, the Python names, the
program's options, the control of the GPU oracle comparison (the float32 statement of tests/score_ref.py on the float32
oracle against the float64 statement on the float64 oracle, under the comparison the GPU test uses) and two mutants of the
float64 statement that the comparison must catch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import score_ref as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
TOP = 4


def test_header_and_python_names():
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header[header.index("int lstm_hip_score("):], flags=re.S)
    decl = decl[:decl.index(";")]
    assert re.sub(r"\s+", " ", decl) == (
        "int lstm_hip_score(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, const float *h0, "
        "const float *c0, const lstm_hip_scoring *opt, const int32_t *start_state , const lstm_hip_scores *out , float *h_out, "
        "float *c_out)"), decl

    def fields(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S)
        assert m, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        return re.findall(r"^\s*(?:const\s+)?(\w+)\s+\*?(\w+);", body, re.M)

    assert fields("lstm_hip_scoring") == [("uint32_t", "size"), ("int32_t", "first"), ("int32_t", "top_n"), ("lstm_hip_constraint", "con")]
    assert fields("lstm_hip_scores") == [("uint32_t", "size"), ("float", "surprisal"), ("float", "entropy"), ("uint8_t", "rank"),
                                         ("uint8_t", "top_byte"), ("float", "top_bits"), ("double", "bits"), ("int32_t", "end_state")]
    assert "lstm_hip_score" in lstm_hip.SYMBOLS and hasattr(lstm_hip.load_library(), "lstm_hip_score")
    assert [f[0] for f in lstm_hip._Scoring._fields_] == ["size", "first", "top_n", "con"]
    assert [f[0] for f in lstm_hip._Scores._fields_] == ["size", "surprisal", "entropy", "rank", "top_byte", "top_bits", "bits", "end_state"]
    assert C.sizeof(lstm_hip._Scoring) == 24 and lstm_hip._Scoring.con.offset == 16  # the C layout on this ABI
    assert C.sizeof(lstm_hip._Scores) == 64 and lstm_hip._Scores.surprisal.offset == 8
    import inspect
    assert list(inspect.signature(lstm_hip.Lstm.score).parameters) == ["self", "texts", "h0", "c0", "first", "top_n", "constraint",
                                                                       "start_state"]
    # the kernel's statistics id is the last one, behind the existing ones
    api = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "lstm_hip_api.cpp")).read()
    enum = api[api.index("enum KernelId {"):api.index("K_COUNT")]
    assert re.findall(r"\bK_\w+", re.sub(r"//.*", "", enum))[-2:] == ["K_BEAM_BACKTRACK", "K_SCORE_HEAD"]
    assert re.search(r'"beam_backtrack",\s*"score_head"\};', api)


def test_program_options():
    out = subprocess.run([GEN, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for flag in ("--score-bytes", "--top"):
        assert flag in out.stdout, flag
    base = [GEN, "--load", "nowhere"]
    for bad in (["--top", "2"], ["--top", "2", "--count", "1"], ["--score", "f", "--top", "2"],       # --top needs --score-bytes
                ["--score-bytes", "f", "--top", "0"], ["--score-bytes", "f", "--top", "9"], ["--score-bytes", "f", "--top", "x"],
                ["--score-bytes"],
                ["--score-bytes", "f", "--count", "1"], ["--score-bytes", "f", "--score", "g"],       # a mode of its own
                ["--score-bytes", "f", "--temperature", "1"], ["--score-bytes", "f", "--streams", "2"],
                ["--score-bytes", "f", "--prime", "a"], ["--score-bytes", "f", "--top-k", "3"],
                ["--score-bytes", "f", "--allow", "65", "--ban", "65"]):                              # nothing left to score under
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
    # good options get past the parser: the checkpoint is what fails (status 1)
    for good in (["--score-bytes", "f"], ["--score-bytes", "f", "--top", "1"], ["--score-bytes", "f", "--top", "8", "--utf8"],
                 ["--score-bytes", "f", "--allow", "0x20-0x7e,10"], ["--score-bytes", "f", "--utf8", "--ban", "0"],
                 ["--top", "3", "--score-bytes", "f", "--stable-softmax"]):
        r = subprocess.run(base + good, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (good, r.returncode, r.stderr)


@pytest.fixture(scope="module")
def case(oracle32, oracle64):
    """the oracle case, first = 0 and first = 1: (float32 statement, float64 statement) of each"""
    N, P, texts, h0, c0 = sc.oracle_case()
    return {first: (sc.score32(oracle32, N, P, texts, h0, c0, first=bool(first), top_n=TOP),
                    sc.score64(oracle64, N, P, texts, h0, c0, first=bool(first), top_n=TOP)) for first in (0, 1)}


@pytest.mark.parametrize("first", [0, 1])
def test_control_of_the_gpu_oracle_comparison(case, first):
    """The float32 statement against the float64 one under sc.compare, the comparison tests/test_score.py holds the device to:
    nothing fails, and on the reference alone the rule leaves out no position (every rank and every top-4 list is equal)."""
    got, want = case[first]
    fig, fails = sc.compare(got, want, bool(first), TOP)
    gap_x, gap_top = np.inf, np.inf
    for s in range(8):
        for j in range(0 if first else 1, 48):
            lnp = want["lnp"][s][j]
            d = np.abs(lnp + want["surprisal"][s][j] * np.log(2.0))
            gap_x = min(gap_x, np.sort(d)[1])
            head = np.sort(lnp)[::-1][:TOP + 1]
            gap_top = min(gap_top, float((head[:-1] - head[1:]).min()))
    print(f"first {first}: surprisal {fig['surprisal']:.3g} entropy {fig['entropy']:.3g} top_bits {fig['top_bits']:.3g} bits; "
          f"left out {fig['left_out_rank']} / {fig['left_out_top']} of {fig['scored']}; nearest ln p to the text byte's {gap_x:.3g}, "
          f"nearest two of the first five {gap_top:.3g}")
    assert fails == [], fails[:5]
    assert fig["scored"] == 8 * (48 if first else 47)
    assert fig["left_out_rank"] == 0 and fig["left_out_top"] == 0
    assert gap_x >= sc.NEAR and gap_top >= sc.NEAR
    for s in range(8):  # ... so every rank and list is equal outright
        lo = 0 if first else 1
        assert np.array_equal(got["rank"][s][lo:], want["rank"][s][lo:]) and np.array_equal(got["top_byte"][s][lo:], want["top_byte"][s][lo:])
    # the case is no easy one: the model is often wrong, and the texts have bytes far down its list
    ranks = np.concatenate([r[1:] for r in want["rank"]])
    assert (ranks == 0).any() and ranks.max() >= 20


def test_the_comparison_leaves_out_near_ties_and_no_more(case):
    got, want = case[1]
    want = dict(want, lnp=[a.copy() for a in want["lnp"]])
    wrong = dict(got, rank=[a.copy() for a in got["rank"]], top_byte=[a.copy() for a in got["top_byte"]])
    s, j = 3, 17
    x_lnp = -want["surprisal"][s][j] * np.log(2.0)
    other = int(np.argsort(np.abs(want["lnp"][s][j] - x_lnp))[1])
    wrong["rank"][s][j] ^= 1
    _, fails = sc.compare(wrong, want, True, TOP)
    assert len(fails) == 1 and "rank" in fails[0], fails
    want["lnp"][s][j][other] = x_lnp + 0.5 * sc.NEAR  # another byte within NEAR of the text byte: the position is left out
    fig, fails = sc.compare(wrong, want, True, TOP)
    assert fails == [] and fig["left_out_rank"] == 1, (fails, fig)
    # the alternatives: a swap of the first two is caught unless two of the first five are near
    got, want = case[1]
    want = dict(want, lnp=[a.copy() for a in want["lnp"]])
    wrong = dict(got, top_byte=[a.copy() for a in got["top_byte"]])
    wrong["top_byte"][s][j][[0, 1]] = wrong["top_byte"][s][j][[1, 0]]
    _, fails = sc.compare(wrong, want, True, TOP)
    assert len(fails) == 1 and "alternatives" in fails[0], fails
    order = np.argsort(want["lnp"][s][j])[::-1]
    want["lnp"][s][j][order[1]] = want["lnp"][s][j][order[0]] - 0.5 * sc.NEAR
    fig, fails = sc.compare(wrong, want, True, TOP)
    assert fails == [] and fig["left_out_top"] == 1, (fails, fig)
    # more than 1 % left out is a failure of its own
    for jj in range(1, 8):
        o = np.argsort(want["lnp"][s][jj])[::-1]
        want["lnp"][s][jj][o[1]] = want["lnp"][s][jj][o[0]] - 0.5 * sc.NEAR
    _, fails = sc.compare(wrong, want, True, TOP)
    assert any("left out" in f for f in fails), fails


@pytest.mark.parametrize("first", [0, 1])
def test_mutants_of_the_statement_are_caught(case, oracle64, first):
    N, P, texts, h0, c0 = sc.oracle_case()
    _, want = case[first]
    late = sc.score64(oracle64, N, P, texts, h0, c0, first=bool(first), top_n=TOP, shift=1)  # byte j on the state after j + 1 inputs
    fig, fails = sc.compare(late, want, bool(first), TOP)
    assert fails and fig["surprisal"] > 1.0, (fig, fails[:3])
    other, _ = case[1 - first]  # `first` ignored: the float32 statement of the other setting
    fig, fails = sc.compare(other, want, bool(first), TOP)
    assert fails, fig
    if first:
        assert fig["surprisal"] > 1.0  # byte 0 was not scored
    else:
        assert any("unscored byte 0" in f for f in fails)
