"""`create_predictor_layer` (model.py:306-319) and `BaseModel.calculate_loss` (model.py:108-119) of the reference as free functions with the same
behaviour, written as lookup tables; `create_encoder_layer` mirrors `create_gnn_layer` (model.py:290-304) over the encoders of encoder.py, and
`create_input_layer` / `create_input_feat` are model.py:268-288 and BaseModel.create_input_feat.  BaseModel itself (split objects, DataLoader epochs)
is not built: trainer.train_linkpred_encoder trains an encoder, trainer.train_teacherGNN_linkpred the teacher GNN, against these predictors and losses."""
import torch

from . import encoder, layer, loss

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


# encoder name (upper case) -> class taking (in_channels, hidden_channels, out_channels, num_layers, dropout)
_ENCODERS = {'SAGE': encoder.SAGEEncoder, 'WSAGE': encoder.WSAGEEncoder, 'GCN': encoder.GCNEncoder, 'MLP': encoder.MLPEncoder}


def create_encoder_layer(input_channels, hidden_channels, num_layers, dropout=0, encoder_name='SAGE', data=None):
    """`create_gnn_layer` over the encoders that are built: SAGE | WSAGE | GCN | MLP, case-insensitive, widths input -> hidden -> ... -> hidden;
    CN | AA | PPR go to Heuristics as in the reference; TRANSFORMER and unknown names raise NotImplementedError."""
    name = str(encoder_name)
    make = _ENCODERS.get(name.upper())
    if make is not None:
        return make(input_channels, hidden_channels, hidden_channels, num_layers, dropout)
    if name in ('CN', 'AA', 'PPR'):
        return layer.Heuristics(name, data)
    if name.upper() == 'TRANSFORMER':
        raise NotImplementedError("encoder_name TRANSFORMER is not built on the HIP path: it needs torch_geometric's TransformerConv (attention over the edges)")
    raise NotImplementedError(f'encoder_name {encoder_name} not implemented')


def create_input_layer(num_nodes, num_node_feats, hidden_channels, use_node_feats=True, train_node_emb=False, pretrain_emb=None):
    """(input_dim, emb): model.py:268-288.  A trainable Embedding(num_nodes, hidden_channels) when the node features are not used, or beside them
    under train_node_emb; a pretrained embedding file is not read here (raises)."""
    if pretrain_emb is not None and pretrain_emb != '':
        raise NotImplementedError('--pretrain_emb is not built on the HIP path: it needs a saved embedding matrix loaded with torch.load')
    emb = None
    if use_node_feats:
        input_dim = num_node_feats
        if train_node_emb:
            emb = torch.nn.Embedding(num_nodes, hidden_channels)
            input_dim += hidden_channels
    else:
        emb = torch.nn.Embedding(num_nodes, hidden_channels)
        input_dim = hidden_channels
    return input_dim, emb


def reset_input_layer(emb):
    """BaseModel.param_init's part for the embedding: xavier_uniform_ on its weight."""
    if emb is not None:
        torch.nn.init.xavier_uniform_(emb.weight)


def create_input_feat(emb, x, use_node_feats=True):
    """BaseModel.create_input_feat (model.py:96-106): data.x, the embedding's weight, or their concatenation [emb.weight | x] (float32)."""
    if use_node_feats:
        feat = x.to(torch.float32)
        if emb is not None:
            feat = torch.cat([emb.weight, feat], dim=-1)
        return feat
    return emb.weight


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
