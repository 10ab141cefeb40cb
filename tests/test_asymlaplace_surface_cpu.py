"""The public surface of the asymmetric Laplace likelihood, checked without a GPU: the enumerator in include/agpl.h, the Python
type and its descriptor, and the headers and documents that have to name the kind."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as fh:
        return fh.read()


def test_header_declares_the_kind():
    h = _read("include", "agpl.h")
    assert re.search(r"\bAGPL_LIK_ASYMLAPLACE\s*=\s*9\b", h)
    assert re.search(r"#define AGPL_VERSION 121\b", h)  # the ABI did not grow
    enum = " ".join(h[h.index("typedef enum {\n    AGPL_LIK_BERNOULLI_LOGISTIC"):h.index("} agpl_lik_kind;")].split())
    tail = enum[enum.index("AGPL_LIK_BINOMIAL = 8"):]
    # the comment says that the reference has no such file and states the tilt identity
    assert "NO file in the reference" in tail
    assert "4 tau (1 - tau) exp(kappa (y - f)) Laplace(y | f; beta = 2 sigma)" in tail and "kappa = (1 - 2 tau) / (2 sigma)" in tail


def test_package_exports_the_likelihood_and_its_descriptor():
    import agpl_amd
    from agpl_amd import likelihoods

    assert "AsymmetricLaplaceLikelihood" in agpl_amd.__all__ and likelihoods.KIND_ASYMLAPLACE == 9
    lik = agpl_amd.AsymmetricLaplaceLikelihood(0.9, 0.7)
    d = lik.desc()
    assert (d.kind, d.nlatent, d.p[0], d.p[1]) == (9, 1, 0.7, 0.9)
    assert lik.ykind == "real" and agpl_amd.nlatent(lik) == 1 and lik._param_names == ("sigma",)
    dflt = agpl_amd.AsymmetricLaplaceLikelihood()
    assert (dflt.tau, dflt.sigma) == (0.5, 1.0)
    assert agpl_amd.AsymmetricLaplaceLikelihood(tau=0.1, sigma=2.0)._params() == (2.0, 0.1)


def test_headers_and_documents_name_the_kind():
    for name in ("agpl_predictive.h", "agpl_quantile.h", "agpl_sample_y.h", "agpl_likgrad.h"):
        assert re.search(r"\bAsymLaplace\(", _read("include", name)), name
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "AGPL_LIK_ASYMLAPLACE" in _read(name), name
    assert re.search(r"^### 4\.30 ", _read("DESIGN.md"), flags=re.M)
    assert "AsymmetricLaplaceLikelihood" in _read("README.md")
    # the header's sampling rule is the inverse distribution function in its log1p forms
    sy = _read("include", "agpl_sample_y.h")
    assert "log1p(d / tau)" in sy and "log1p(-d / (1 - tau))" in sy
