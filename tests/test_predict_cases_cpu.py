"""The cases of the pool-scoring tests, checked on the CPU so that the GPU tests cannot hide a failure behind a bad case:
every K~ is well conditioned, every reference variance is positive, the truncated basis is orthonormal, and the
re-associated form the device evaluates (predict_cases.moments_reassociated, numpy fp64) agrees with the long-double
restatement of lambda_moments_star to 1e-12 and with oracle.predict_moments to 1e-10 (both relative to max |.|)."""
import numpy as np
import pytest

import predict_cases as cases


@pytest.mark.parametrize("shape", cases.CASES, ids=lambda s: "P{}-nt{}-k{}-px{}".format(*s))
def test_case_is_sound(shape):
    c = cases.make_case(*shape)
    P, nt, k, px = shape
    assert c["xstar"].shape == (P, px * px) and c["xtilde"].shape == (nt, px * px) and c["K"].shape == (k, k)
    cond = np.linalg.cond(c["K"])
    mu_ref, s2_ref = cases.reference(*shape)
    print(f"{shape}: d = {c['d']}, cond(K~_b) = {cond:.2e}, sigma2_ref in [{float(s2_ref.min()):.3f}, {float(s2_ref.max()):.3f}]")
    assert cond <= 1e5
    assert np.all(s2_ref > 0)
    assert np.linalg.eigvalsh(c["V"]).min() > 0
    if c["B"] is not None:
        assert np.max(np.abs(c["B"].T @ c["B"] - np.eye(k))) <= 1e-13
    else:
        assert k == nt


def test_first_case_keeps_every_pixel_of_a_6x6_image():
    """d = 36 is the point of the case: a pixel count that is no multiple of the GEMM's k step."""
    assert cases.make_case(*cases.CASES[0])["d"] == 36


@pytest.mark.parametrize("shape", cases.CASES, ids=lambda s: "P{}-nt{}-k{}-px{}".format(*s))
def test_reassociated_form_matches_the_references(shape):
    c = cases.make_case(*shape)
    mu_ref, s2_ref = cases.reference(*shape)
    mu, s2 = cases.moments_reassociated(c)
    mu_o, s2_o = cases.moments_oracle(c)
    e = (cases.err(mu, mu_ref), cases.err(s2, s2_ref), cases.err(mu_o, mu_ref), cases.err(s2_o, s2_ref))
    print(f"{shape}: re-associated vs long double mu {e[0]:.2e} sigma2 {e[1]:.2e}; oracle vs long double mu {e[2]:.2e} sigma2 {e[3]:.2e}")
    assert e[0] <= 1e-12 and e[1] <= 1e-12
    assert cases.err(mu, mu_o) <= 1e-10 and cases.err(s2, s2_o) <= 1e-10
