"""``Demix.Traces`` (the reference's module name); the implementation lives in dnmf_amd."""
from dnmf_amd.Demix.Traces import cleanTraces, deconvolveTraces, detrend_df_f, histogram_match  # noqa: F401
