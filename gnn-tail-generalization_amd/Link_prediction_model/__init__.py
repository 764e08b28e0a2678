"""The decoder side of the reference's link-prediction experiment (Link_prediction_model/layer.py, loss.py, model.py) on the HIP path: the DOT and
MLP predictors with a fused entry on index pairs, the five pairwise losses, and BaseModel's two dispatch functions.  Not built: the PyG encoders,
the other predictors, edge_LP.py, the BaseModel training loop (trainer.train_teacherGNN_linkpred trains the teacher against these instead)."""
from .layer import (GCN, MLP, SAGE, WSAGE, BilinearPredictor, DotPredictor, Heuristics, MLPBilPredictor, MLPCatPredictor, MLPDotPredictor,  # noqa: F401
                    MLPPredictor, Transformer)
from .loss import adaptive_auc_loss, auc_loss, ce_loss, info_nce_loss, log_rank_loss  # noqa: F401
from .model import calculate_loss, create_predictor_layer  # noqa: F401
