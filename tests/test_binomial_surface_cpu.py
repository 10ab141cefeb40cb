"""The public surface of the binomial likelihood, checked without a GPU: the enumerator in include/agpl.h, the Python type and
its descriptor, and the headers and documents that have to name the kind."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as fh:
        return fh.read()


def test_header_declares_the_kind():
    h = _read("include", "agpl.h")
    assert re.search(r"\bAGPL_LIK_BINOMIAL\s*=\s*8\b", h)
    assert re.search(r"#define AGPL_VERSION 121\b", h)  # the ABI did not grow
    enum = h[h.index("typedef enum {\n    AGPL_LIK_BERNOULLI_LOGISTIC"):h.index("} agpl_lik_kind;")]
    assert "no file in the reference" in " ".join(enum.split()).lower() and "PG(n" in enum


def test_package_exports_the_likelihood_and_its_descriptor():
    import agpl_amd
    from agpl_amd import likelihoods

    assert "BinomialLikelihood" in agpl_amd.__all__ and likelihoods.KIND_BINOMIAL == 8
    lik = agpl_amd.BinomialLikelihood(12)
    d = lik.desc()
    assert (d.kind, d.nlatent, d.p[0]) == (8, 1, 12.0)
    assert lik.ykind == "i32" and agpl_amd.nlatent(lik) == 1 and lik._param_names == ()
    assert agpl_amd.BinomialLikelihood().n == 1


def test_headers_and_documents_name_the_kind():
    for name in ("agpl_predictive.h", "agpl_quantile.h", "agpl_sample_y.h", "agpl_likgrad.h"):
        assert re.search(r"\bBinomial\(n\)", _read("include", name)), name
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "AGPL_LIK_BINOMIAL" in _read(name), name
    design = _read("DESIGN.md")
    assert re.search(r"^### 4\.28 ", design, flags=re.M)
    # the header's sampling rule states its switch point and the largest n it serves
    sy = _read("include", "agpl_sample_y.h")
    assert "n <= 64" in sy and "2^22" in sy
