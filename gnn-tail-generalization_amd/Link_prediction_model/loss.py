"""The pairwise losses of the reference's Link_prediction_model/loss.py under its names and signatures, on ops.rank_loss (csrc/cb_linkpred.hip): every
term in float64 from the fp32 scores by the formula as written, summed in one fixed order, rounded once.  pos_out holds P scores and neg_out
P * num_neg, read as [P, num_neg] exactly as the reference reshapes them; both may carry the trailing 1 of MLPPredictor's output.
Deviation: the reference evaluates in fp32, where `1 - sigmoid(s)` cancels (ce_loss) and `exp(s)` overflows above s = 88 (info_nce_loss); the
value here is the float64 one.  ce_loss of the reference takes any two lengths; here len(neg_out) must be a multiple of len(pos_out)."""
from .. import ops


def auc_loss(pos_out, neg_out, num_neg):
    return ops.rank_loss('auc_loss', pos_out, neg_out, num_neg)


def adaptive_auc_loss(pos_out, neg_out, num_neg, weight):
    return ops.rank_loss('adaptive_auc_loss', pos_out, neg_out, num_neg, weight)


def log_rank_loss(pos_out, neg_out, num_neg):
    return ops.rank_loss('log_rank_loss', pos_out, neg_out, num_neg)


def ce_loss(pos_out, neg_out):
    return ops.rank_loss('ce_loss', pos_out, neg_out, None)


def info_nce_loss(pos_out, neg_out, num_neg):
    return ops.rank_loss('info_nce_loss', pos_out, neg_out, num_neg)
