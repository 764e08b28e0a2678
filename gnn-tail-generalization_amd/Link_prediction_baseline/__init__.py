"""The reference's link-prediction baselines (Link_prediction_baseline/heuristics.py) on the device CSR."""
from .heuristics import AA, CN, PPR, eva_heuristics_v2_dec25, tonp  # noqa: F401
