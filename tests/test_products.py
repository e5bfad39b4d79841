"""The window's dense products and bf16 packers, each on its own (-m gpu): gemm / gemm_slabs / gemm_fold, gemm_bf16,
transpose_pack_bf16 and pack_bf16 called directly through the driver eigen-lstm_amd/product_check (tests/product_check.hip),
on the cases, operands and checks of tests/product_cases.py; tests/test_products_cpu.py is the control without a GPU.

One driver process per test, never two at a time, each under a time limit of its own.  The driver dumps whole allocations and
judges nothing; every check is here.  After the first abnormal driver exit (a signal, a time limit, a HIP error) every later
test of the module fails at once without starting the driver again.

Every fp32 family runs under both tile rules (LSTM_HIP_GEMM_SMALL_TILES unset and =0: the variable is read once per process)
and every bf16 family under LSTM_HIP_BF16_GEMM_TILE=64 and =128; test_products_cpu.py asserts from the shape rule that this
reaches all five instantiations of k_gemm_regs and both tiles of k_gemm_bf16.

Measured on an MI355X (256 CUs; every case: profiles/products/accuracy.jsonl, written with
PRODUCTS_REPORT=profiles/products/accuracy.jsonl pytest -m gpu tests/test_products.py): every exact case bit-identical.
e in units of 2^-24 sum|a b|, kernel against the ascending float32 loop:
                                             RMS kernel / loop      max kernel / loop
  fp32 K = 9 (one group and a tail)             0.47 / 0.52            3.3 / 3.6
  fp32 K = 64 ... 1040, one slab                0.24 - 0.28 / 0.47     1.2 - 1.7 / 2.9 - 4.1
  fp32 K = 72 ... 531, 2 - 3 slabs              0.15 - 0.24 / 0.47     0.7 - 1.4 / 3.6 - 4.6
  fp32 headline dU (2 slabs) / dWhy (16)        0.17, 0.07 / 0.48      0.63, 0.24 / 3.3, 2.6
  fp32 headline Y / DHy                         0.24 / 0.47            1.3, 1.2 / 3.5, 3.3
  bf16 K = 256 ... 320, 1 - 3 slabs             0.10 - 0.14 / 0.18     0.6 - 1.6 / 1.4 - 1.8
  bf16 headline dU (4 slabs) / dWhy (15)        0.08, 0.05 / 0.26      0.41, 0.19 / 1.6, 1.8
The two tile rules give the same figures (the order of an output's sum does not depend on the tile).  The module takes 14 s.
"""
import json
import os
import subprocess
import time

import numpy as np
import pytest

import product_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "eigen-lstm_amd", "product_check")
REPORT = os.environ.get("PRODUCTS_REPORT")  # a file to append one JSON line per accuracy case to (profiles/products)
TILE_ENV = ("LSTM_HIP_GEMM_SMALL_TILES", "LSTM_HIP_BF16_GEMM_TILE")

_abnormal = None        # the first abnormal driver exit of this module: nothing more is started after it


def _report(rec):
    print(rec)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(rec) + "\n")


def run_driver(tmp_path, jobs, env=None, reps=2, timeout=9.5, lines=()):
    """One driver process over `jobs`; returns the run (product_cases docstring)."""
    global _abnormal
    if _abnormal:
        pytest.fail(f"not started: an earlier driver process of this module ended abnormally ({_abnormal})")
    assert os.path.exists(DRIVER), f"{DRIVER} is not built (make -C eigen-lstm_amd/csrc)"
    with open(tmp_path / "manifest.txt", "w") as f:
        f.writelines(line + "\n" for line in lines)
        for job in jobs:
            f.write(pc.manifest_line(job, reps) + "\n")
            job.A.tofile(tmp_path / f"{job.id}.A")
            if job.B is not None:
                job.B.tofile(tmp_path / f"{job.id}.B")
    e = {k: v for k, v in os.environ.items() if k not in TILE_ENV}
    e.update(env or {})
    t0 = time.time()
    try:
        done = subprocess.run([DRIVER, str(tmp_path)], env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _abnormal = f"time limit of {timeout} s"
        pytest.fail(f"product_check ran into its {_abnormal}")
    if done.returncode != 0:
        if done.returncode != 2:            # 2: the driver refused the manifest before launching anything -- a bug of the test
            _abnormal = f"exit status {done.returncode}: {done.stderr.strip()[-300:]}"
        pytest.fail(f"product_check exit status {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-2000:]}")
    run = dict(out={}, results={}, seconds=time.time() - t0)
    with open(tmp_path / "results.txt") as f:
        for line in f:
            w = line.split()
            if w[0] == "n_cus":
                run["results"]["n_cus"] = int(w[1])
            else:
                run["results"][(w[0], int(w[1]), w[2])] = int(w[3])
    for job in jobs:
        for buf in ("C", "S"):
            for rep in range(reps):
                path = tmp_path / f"{job.id}.{buf}.r{rep}"
                if path.exists():
                    run["out"][(job.id, buf, rep)] = path.read_bytes()
    return run


EXACT = [("kss", {}), ("kss", {"LSTM_HIP_GEMM_SMALL_TILES": "0"}), ("ksf", {}), ("ksf", {"LSTM_HIP_GEMM_SMALL_TILES": "0"}),
         ("kff", {}), ("kff", {"LSTM_HIP_GEMM_SMALL_TILES": "0"}), ("fold", {}),
         ("bf16", {"LSTM_HIP_BF16_GEMM_TILE": "64"}), ("bf16", {"LSTM_HIP_BF16_GEMM_TILE": "128"}), ("tpack", {}), ("pack", {})]


def _env_id(env):
    return "-".join(f"{k.split('_')[-1].lower()}{v}" for k, v in env.items()) or "default"


@pytest.mark.parametrize("family,env", EXACT, ids=[f"{f}-{_env_id(e)}" for f, e in EXACT])
def test_exact(family, env, tmp_path):
    """Integer operands: C and every slab bit for bit the int64 product, sentinels intact, every element written, the count of
    slabs as recomputed, two runs in one process identical (product_cases.check_exact)."""
    jobs = [pc.make_job(c) for c in pc.FAMILIES[family]]
    run = run_driver(tmp_path, jobs, env)
    for job in jobs:
        pc.check_exact(job, run)


@pytest.mark.parametrize("case", pc.REAL_FP32 + pc.REAL_BF16, ids=lambda c: c.id)
def test_exact_at_the_headline_shape(case, tmp_path):
    """Np 512, S 100, B 64 with the splits the library's rule picks for this device (and the rule as restated in
    product_cases for its CU count); the tile is the rule's own."""
    job = pc.make_job(case)
    pc.check_exact(job, run_driver(tmp_path, [job]))


ACCURACY = [("fp32", pc.ACC_FP32, {}), ("fp32", pc.ACC_FP32, {"LSTM_HIP_GEMM_SMALL_TILES": "0"}),
            ("bf16", pc.ACC_BF16, {"LSTM_HIP_BF16_GEMM_TILE": "64"}), ("bf16", pc.ACC_BF16, {"LSTM_HIP_BF16_GEMM_TILE": "128"})]


def _accuracy(jobs, run, env):
    failures = []
    for job in jobs:
        C, _, used, _ = pc.check_product_layout(job, run, 0)
        fig = pc.accuracy_figures(job, C)
        _report(dict(case=job.id, what=job.what, env=env, slabs=used, n_cus=run["results"]["n_cus"], **fig))
        try:
            pc.assert_accuracy(job, fig)
        except AssertionError as err:
            failures.append(str(err))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name,cases,env", ACCURACY, ids=[f"{n}-{_env_id(e)}" for n, _, e in ACCURACY])
def test_accuracy(name, cases, env, tmp_path):
    """N(0,1) operands: RMS and max of e = |C - ref64| / (2^-24 sum |a b|) against the ascending float32 loop's, margins 1.25
    and 2 (product_cases.assert_accuracy)."""
    jobs = [pc.make_job(c, "accuracy") for c in cases]
    _accuracy(jobs, run_driver(tmp_path, jobs, env, reps=1), env)


@pytest.mark.parametrize("case", pc.REAL_FP32 + pc.REAL_BF16, ids=lambda c: c.id)
def test_accuracy_at_the_headline_shape(case, tmp_path):
    """The same on a 64 x 64 sample of the outputs (product_cases.sample_of), kernel and yardstick over the same outputs."""
    if case.kind == "gemm_slabs":            # no C of its own: fold the slabs it returns, as the update launch does
        case = case._replace(p=dict(case.p, fold=1), id=case.id + "-fold")
    job = pc.make_job(case, "accuracy")
    _accuracy([job], run_driver(tmp_path, [job], reps=1), {})


def test_shape_rules_are_static(tmp_path):
    """gemm_pick_splits / gemm_bf16_pick_splits return the same value on repeated calls, and equal the rule restated in
    product_cases for the device's CU count; the calls that take that value report as many slabs after recomputation (the
    headline tests: gemm_slabs' return value, the slabs written by gemm and gemm_bf16)."""
    shapes = [("dU", 0, 0, 1, 2048, 512, 6336), ("dWhy", 0, 0, 1, 256, 512, 6336), ("Y", 0, 0, 0, 256, 6336, 512),
              ("DHy", 0, 1, 0, 512, 6336, 256), ("dU-b", 1, 0, 0, 2048, 512, 6336), ("dWhy-b", 1, 0, 0, 256, 512, 6336),
              ("dU-small", 0, 0, 1, 320, 80, 531), ("dU-1024", 0, 0, 1, 4096, 1024, 1584), ("dWhy-b-small", 1, 0, 0, 256, 128, 320)]
    run = run_driver(tmp_path, [], lines=[f"pick_splits {name} bf16={bf16} TA={TA} TB={TB} M={M} Nn={Nn} K={K}"
                                          for name, bf16, TA, TB, M, Nn, K in shapes])
    n_cus = run["results"]["n_cus"]
    for name, bf16, TA, TB, M, Nn, K in shapes:
        first, second = run["results"][(name, 0, "pick0")], run["results"][(name, 0, "pick1")]
        rule = pc.bf16_pick_splits(M, Nn, K) if bf16 else pc.regs_pick_splits(bool(TA), not TB, M, Nn, K, n_cus)
        assert first == second == rule, (name, first, second, rule, n_cus)
        used = (pc.bf16_plan(M, Nn, K, first) if bf16 else pc.regs_plan(bool(TA), not TB, M, Nn, K, first))[0]
        # (bf16: an upper bound -- whole k-tiles per slab make 15 slabs of the 16 at the headline dWhy; product_cases.expected_used)
        assert used <= first if bf16 else used == first, f"{name}: the rule picks {first} slabs, a call with that request uses {used}"
