"""The decoder side of the reference's link-prediction experiment (Link_prediction_model/layer.py, loss.py, model.py) on the HIP path: the DOT and
MLP predictors with a fused entry on index pairs, the five pairwise losses, BaseModel's dispatch functions, and the encoders it trains — SAGEEncoder,
WSAGEEncoder, GCNEncoder (one fused aggregation + GEMM kernel per layer, ops.sage_layer) and MLPEncoder, built by create_encoder_layer over
create_input_layer's trainable embedding (trainer.train_linkpred_encoder), and TransformerEncoder (one stacked GEMM and one attention kernel over the
CSR rows per layer, ops.transformer_conv), which the trainer builds for `args.encoder = 'TRANSFORMER'`.  `SAGE` / `WSAGE` / `GCN` / `MLP` /
`Transformer` themselves stand for the torch_geometric modules and keep raising.  The BIL / MLPDOT / MLPBIL / MLPCAT predictors are built in
pair_predictor.py under names of their own (BilinearPairPredictor, MLPDotPairPredictor, MLPBilPairPredictor, MLPCatPairPredictor; fused entries
ops.rows_linear / ops.pair_bilinear) with create_pair_predictor_layer over all six names; layer.py's `BilinearPredictor` / `MLP*Predictor` names and
create_predictor_layer's four entries for them keep raising.  Not built: edge weights for GraphConv, edge_LP.py, BaseModel's split objects and
DataLoader epochs (trainer.train_teacherGNN_linkpred trains the teacher against the same predictors instead)."""
from .layer import (GCN, MLP, SAGE, WSAGE, BilinearPredictor, DotPredictor, Heuristics, MLPBilPredictor, MLPCatPredictor, MLPDotPredictor,  # noqa: F401
                    MLPPredictor, Transformer)
from .loss import adaptive_auc_loss, auc_loss, ce_loss, info_nce_loss, log_rank_loss  # noqa: F401
from .encoder import GCNEncoder, MLPEncoder, SAGEEncoder, TransformerConv, TransformerEncoder, WSAGEEncoder  # noqa: F401
from . import pair_predictor  # noqa: F401
from .pair_predictor import (BilinearPairPredictor, MLPBilPairPredictor, MLPCatPairPredictor, MLPDotPairPredictor,  # noqa: F401
                             create_pair_predictor_layer)
from .model import calculate_loss, create_encoder_layer, create_input_feat, create_input_layer, create_predictor_layer  # noqa: F401
