"""CPU-only: the leave-one-out predictive's C-ABI entry points are exported by the built library and declared to ctypes, and its
result type is part of the package's public surface."""


def test_loo_entry_points_exported(hiplib):
    from ppca_rs_amd import _lib

    for name in ("ppca_loo_predictive", "ppca_mix_loo_predictive"):
        assert hasattr(hiplib, name), name
        assert name in _lib.SIGNATURES, name
    assert hiplib.ppca_abi_version() == 6


def test_loo_python_surface():
    import ppca_rs_amd as p

    assert "LooPredictive" in p.__all__
    for cls in (p.PPCAModel, p.PPCAMix):
        for meth in ("loo_predictive", "loo_llks", "loo_llk"):
            assert callable(getattr(cls, meth, None)), (cls.__name__, meth)
    for meth in ("mean", "variance", "llks", "llk", "zscores"):
        assert callable(getattr(p.LooPredictive, meth, None)), meth
