"""Correct & Smooth / label propagation on the HIP aggregation path — the names and signatures of the reference's
Label_propagation_model package (outcome_correlation.py, LP_Adj.py: LPStep).  PreStep (spectral / community features need external solvers),
MidStep's MLP and LabelPropagation_Adj are not built."""
from .outcome_correlation import (ADJ_FORMS, Clamp, FixRows, Identity, NormalizedAdj, double_correlation_autoscale, double_correlation_fixed,  # noqa: F401
                                  gen_normalized_adjs, general_outcome_correlation, get_labels_from_name, label_propagation,
                                  only_outcome_correlation, pre_outcome_correlation, pre_residual_correlation, process_adj)
from .LP_Adj import LPStep  # noqa: F401
