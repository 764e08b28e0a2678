"""`create_predictor_layer` (model.py:306-319) and `BaseModel.calculate_loss` (model.py:108-119) of the reference as free functions with the same
behaviour, written as lookup tables.  BaseModel itself (PyG encoders, split objects, DataLoader epochs) is not built:
trainer.train_teacherGNN_linkpred trains the teacher GNN against these predictors and losses."""
from . import layer, loss

# predictor name (upper case) -> constructor from (hidden_channels, num_layers, dropout)
_PREDICTORS = {
    'DOT': lambda c, n, p: layer.DotPredictor(),
    'BIL': lambda c, n, p: layer.BilinearPredictor(c),
    'MLP': lambda c, n, p: layer.MLPPredictor(c, c, 1, n, p),
    'MLPDOT': lambda c, n, p: layer.MLPDotPredictor(c, 1, n, p),
    'MLPBIL': lambda c, n, p: layer.MLPBilPredictor(c, 1, n, p),
    'MLPCAT': lambda c, n, p: layer.MLPCatPredictor(c, c, 1, n, p),
}


def create_predictor_layer(hidden_channels, num_layers, dropout=0, predictor_name='MLP'):
    """The predictor `--predictor` names, case-insensitive; an unknown name raises (the reference returns None)."""
    make = _PREDICTORS.get(predictor_name.upper())
    if make is None:
        raise NotImplementedError(f'predictor_name {predictor_name.upper()} not implemented')
    return make(hidden_channels, num_layers, dropout)


def calculate_loss(loss_func_name, pos_out, neg_out, num_neg, margin=None):
    """BaseModel.calculate_loss with self.loss_func_name as the first argument.  ce_loss takes no num_neg; adaptive_auc_loss applies only with a
    margin; every other name — 'AUC' among them — is auc_loss."""
    if loss_func_name == 'ce_loss':
        return ce_loss(pos_out, neg_out)
    if loss_func_name == 'adaptive_auc_loss' and margin is not None:
        return adaptive_auc_loss(pos_out, neg_out, num_neg, margin)
    fn = {'info_nce_loss': info_nce_loss, 'log_rank_loss': log_rank_loss}.get(loss_func_name, auc_loss)
    return fn(pos_out, neg_out, num_neg)


# module-level names, looked up at call time
adaptive_auc_loss, auc_loss, ce_loss, info_nce_loss, log_rank_loss = (loss.adaptive_auc_loss, loss.auc_loss, loss.ce_loss, loss.info_nce_loss,
                                                                     loss.log_rank_loss)
