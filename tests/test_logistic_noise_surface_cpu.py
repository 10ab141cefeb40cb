"""The public surface of the logistic-noise likelihood, checked without a GPU: the enumerator in include/agpl.h, the Python type
and its descriptor, the one parameter check in agpl_lik_desc.h, and the headers and documents that have to name the kind."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as fh:
        return fh.read()


def test_header_declares_the_kind():
    h = _read("include", "agpl.h")
    assert re.search(r"\bAGPL_LIK_LOGISTIC_NOISE\s*=\s*10\b", h)
    assert re.search(r"#define AGPL_VERSION 121\b", h)  # the ABI did not grow
    enum = " ".join(h[h.index("typedef enum {\n    AGPL_LIK_BERNOULLI_LOGISTIC"):h.index("} agpl_lik_kind;")].split())
    tail = enum[enum.index("AGPL_LIK_ASYMLAPLACE = 9"):]
    assert "NO file in the reference" in tail and "E_{omega ~ PG(2,0)} exp(-omega z^2 / 2)" in tail and "PG(2, |y - f| / s)" in tail


def test_package_exports_the_likelihood_and_its_descriptor():
    import agpl_amd
    from agpl_amd import likelihoods, operators

    assert "LogisticNoiseLikelihood" in agpl_amd.__all__ and likelihoods.KIND_LOGISTIC_NOISE == 10
    lik = agpl_amd.LogisticNoiseLikelihood(0.7)
    d = lik.desc()
    assert (d.kind, d.nlatent, d.p[0], d.p[1]) == (10, 1, 0.7, 0.0)
    assert lik.ykind == "real" and agpl_amd.nlatent(lik) == 1 and lik._param_names == ("scale",) and lik._params() == (0.7,)
    assert agpl_amd.LogisticNoiseLikelihood().scale == 1.0
    assert operators._POSTERIOR_FIELDS[likelihoods.KIND_LOGISTIC_NOISE] == ("c",)


def test_the_parameter_check_is_stated_once():
    csrc = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
    every = {name: _read("augmentedgplikelihoods.jl_amd", "csrc", name) for name in sorted(os.listdir(csrc)) if name.endswith((".h", ".hip"))}
    # the predicate and its message: once in all of csrc/, in the header of the shared descriptor check
    for stated in ("bool agpl_logistic_noise_ok(double scale)", "#define AGPL_LOGISTIC_NOISE_MSG"):
        assert [name for name, src in every.items() for _ in range(src.count(stated))] == ["agpl_lik_desc.h"], stated
    assert [name for name, src in every.items() if "agpl_logistic_noise_ok(" in src or "AGPL_LOGISTIC_NOISE_MSG" in src] == ["agpl_lik_desc.h"]
    for name in ("agpl_core.hip", "agpl_predictive.hip", "agpl_quantile.hip", "agpl_sample_y.hip", "agpl_likgrad.hip"):
        assert "LogisticNoise needs" not in every[name] and "AGPL_LIK_CHECK(ctx, lik);" in every[name], name
    assert "agpl_lik_desc_check((lik)" in every["agpl_common.h"]  # what AGPL_LIK_CHECK calls


def test_headers_and_documents_name_the_kind():
    for name in ("agpl_predictive.h", "agpl_quantile.h", "agpl_sample_y.h", "agpl_likgrad.h"):
        assert re.search(r"\bLogisticNoise\(", _read("include", name)), name
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "AGPL_LIK_LOGISTIC_NOISE" in _read(name), name
    assert re.search(r"^### 4\.31 ", _read("DESIGN.md"), flags=re.M)
    assert "LogisticNoiseLikelihood" in _read("README.md")
    assert "log u - log1p(-u)" in _read("include", "agpl_sample_y.h")
