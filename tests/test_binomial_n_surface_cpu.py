"""The public surface of the binomial likelihood with per-point trial counts, checked without a GPU: the enumerator in
include/agpl.h and its stated layout, the Python type, the helper that builds the [N, 2] observation and what it refuses, the
maps from the observation kind to a dtype, and the libraries that did not grow."""
import os
import re

import pytest

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd")


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as fh:
        return fh.read()


def test_header_declares_the_kind_and_its_layout():
    h = _read("include", "agpl.h")
    assert re.search(r"\bAGPL_LIK_BINOMIAL_N\s*=\s*11\b", h)
    assert re.search(r"#define AGPL_VERSION 121\b", h)  # the ABI did not grow
    enum = " ".join(h[h.index("typedef enum {\n    AGPL_LIK_BERNOULLI_LOGISTIC"):h.index("} agpl_lik_kind;")].split())
    assert "int32 [N][2]" in enum and "column 1" in enum and "[N][L]" in enum and "2^22" in enum
    assert "int32 [N][2]" in " ".join(h[:h.index("#ifndef AGPL_H")].split())  # beside the conventions' other layouts of y
    assert len(S.arguments(os.path.join(ROOT, "include", "agpl.h"))) == 45


def test_package_exports_the_likelihood_and_its_descriptor():
    import agpl_amd
    from agpl_amd import likelihoods

    assert "BinomialTrialsLikelihood" in agpl_amd.__all__ and "binomial_obs" in agpl_amd.__all__
    assert likelihoods.KIND_BINOMIAL_N == 11 and likelihoods.KIND_BINOMIAL == 8
    lik = agpl_amd.BinomialTrialsLikelihood()
    d = lik.desc()
    assert (d.kind, d.nlatent) == (11, 1) and list(d.p) == [0.0] * 4
    assert lik.ykind == "i32x2" and agpl_amd.nlatent(lik) == 1 and lik._param_names == () and lik._params() == ()


def test_binomial_obs_builds_the_block_and_names_what_it_refuses():
    torch = pytest.importorskip("torch")
    import agpl_amd

    obs = agpl_amd.binomial_obs(torch.tensor([0, 3, 5]), torch.tensor([1, 3, 4194303]))
    assert obs.dtype == torch.int32 and obs.shape == (3, 2) and obs.is_contiguous()
    assert obs.tolist() == [[0, 1], [3, 3], [5, 4194303]]  # (a count above its trials is data: -inf densities, not an error)
    for y, n, where in (([0, -1, 2], [1, 2, 3], r"y\[1\]"), ([0, 1, 2], [1, 0, 3], r"trials\[1\]"), ([0, 1, 2], [1, 2, 4194304], r"trials\[2\]"),
                        ([0, 1.5], [2, 2], r"y\[1\]"), ([0, 1], [2, 2.5], r"trials\[1\]")):
        with pytest.raises(agpl_amd.ArgumentError, match=where):
            agpl_amd.binomial_obs(torch.tensor(y), torch.tensor(n))
    with pytest.raises(agpl_amd.ArgumentError, match="one length"):
        agpl_amd.binomial_obs(torch.tensor([0, 1]), torch.tensor([1, 2, 3]))


def test_every_map_from_the_observation_kind_knows_the_new_one():
    torch = pytest.importorskip("torch")
    import agpl_amd
    from agpl_amd import operators

    lik = agpl_amd.BinomialTrialsLikelihood()
    assert operators._ydtype(lik, torch.float64) is torch.int32 and operators._ycols(lik) == 2
    assert operators._ycols(agpl_amd.BinomialLikelihood(3)) == 1 and operators._ycols(agpl_amd.CategoricalLikelihood(4)) == 4
    assert operators._POSTERIOR_FIELDS[11] == ("c",)
    with pytest.raises(agpl_amd.ArgumentError, match="trials"):  # refused before any device call
        agpl_amd.synth_xy(lik, 1, 0, 8, ctx=object())
    with pytest.raises(agpl_amd.ArgumentError, match="trials= is for"):
        operators.obs_at(agpl_amd.BinomialLikelihood(3), None, torch.tensor([1]), "predict_y")
    with pytest.raises(agpl_amd.ArgumentError, match="needs trials="):
        operators.obs_at(lik, None, None, "predict_y")
    y, want = operators.obs_at(lik, None, torch.tensor([2, 5]), "predict_y")
    assert y.tolist() == [[0, 2], [0, 5]] and want is False


def test_the_pinned_libraries_did_not_grow():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    assert S.exports(_ffi.SY_LIB_PATH) == ["agpl_sample_y"]
    assert S.exports(_ffi.QT_LIB_PATH) == ["agpl_predictive_cdf", "agpl_predictive_quantile"]
    assert len(S.exports(_ffi.LIB_PATH)) == 45 and len(_ffi.LIBRARIES) == 16


def test_the_rules_name_the_kind_once_per_rule():
    rules = open(os.path.join(PKG, "csrc", "agpl_lik_rules.h")).read()
    # the kind is named once in the one list of kinds, and the device switch expands that list
    desc = open(os.path.join(PKG, "csrc", "agpl_lik_desc.h")).read()
    kinds = re.search(r"#define AGPL_LIK_KINDS\(X\)((?:[^\n]*\\\n)+[^\n]*)\n", desc).group(1)
    assert kinds.count("X(AGPL_LIK_BINOMIAL_N)") == 1 and desc.count("#define AGPL_LIK_KINDS(") == 1
    dispatch = rules[rules.index("void lik_dispatch("):rules.index("ald_beta")]
    assert dispatch.count("AGPL_LIK_KINDS(AGPL_LIK_CASE_)") == 1 and "AGPL_LIK_CASE_(AGPL_LIK_" not in rules
    assert "binomial_n<T>(lik, y)" in rules
    assert re.search(r"lik_needs_y\(int kind\) \{[^}]*AGPL_LIK_BINOMIAL_N", rules)
    common = open(os.path.join(PKG, "csrc", "agpl_common.h")).read()
    assert common.count("binomial_trials(T n)") == 1  # the domain 1 <= n < 2^22 is stated once
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "AGPL_LIK_BINOMIAL_N" in _read(name), name
    assert re.search(r"^### 4\.33 ", _read("DESIGN.md"), flags=re.M)
