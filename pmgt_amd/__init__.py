"""pmgt_amd — MI355X-native PMGT pre-training hot path (HIP kernels behind the reference's Python surface)."""
from .configuration_pmgt import PMGTConfig  # noqa: F401
# (binds the name `recommend` to the function: the submodule stays reachable as `from pmgt_amd.recommend import ...`)
from .recommend import DcnScorer, NcfModelScorer, ncf_head_host, recommend, topk_host  # noqa: F401
from .ncf_train import (NcfHeadTrainer, fit_ncf, ncf_dropout_keep, ncf_dropout_masks, ncf_head_grad_host, ng_sample,  # noqa: F401
                        normalize_item_table)
from .dcn_head import check_dcn_covered, dcn_dropout_masks, dcn_head_grad_host, dcn_head_host, dcn_layout, dcn_scores_host  # noqa: F401
from .dcn import DCN  # noqa: F401
from .dcn_train import DcnGrad, DcnTrainer, evaluate_ctr, fit_dcn  # noqa: F401
from .ncf_model import check_ncf_model_covered, ncf_model_grad_host, ncf_model_layout, ncf_model_scores_host  # noqa: F401
from .ncf_model_train import NcfModelGrad, NcfModelTrainer, fit_ncf_model  # noqa: F401
from .ncf_head import ncf_head_rows_grad_host  # noqa: F401
from .finetune import PmgtNcfOptionsTrainer, PmgtNcfTrainer, finetune_batches, fit_pmgt_ncf  # noqa: F401
from .pair_train import pair_schedule_steps, sgd_step_host  # noqa: F401
from .catalogue_eval import (CatalogueMetrics, HeldoutRanks, catalogue_metrics_host, evaluate_catalogue, heldout_csr,  # noqa: F401
                             heldout_ranks_host)
from .item_graph import ItemGraph, build_item_graph, item_graph_host, synthetic_interactions  # noqa: F401
from .similar import ItemSimScorer, edges_csr, evaluate_neighbours, holdout_edges, item_sim_host, similar_items  # noqa: F401
from .history import HistoryScorer, evaluate_history, history_scores_host, recommend_from_history  # noqa: F401
from .item_knn import (ItemKnnIndex, ItemKnnScorer, build_item_knn, decay_weights, evaluate_item_knn, item_knn_scores_host,  # noqa: F401
                       recommend_item_knn, weighted_history_csr)

__all__ = ["PMGTConfig", "recommend", "topk_host", "ncf_head_host", "ncf_head_grad_host", "ng_sample", "NcfHeadTrainer", "fit_ncf",
           "normalize_item_table", "ncf_dropout_keep", "ncf_dropout_masks", "DCN", "DcnGrad", "DcnTrainer", "evaluate_ctr", "fit_dcn",
           "check_dcn_covered", "dcn_layout", "dcn_head_host", "dcn_head_grad_host", "dcn_dropout_masks", "ncf_head_rows_grad_host", "PmgtNcfTrainer", "PmgtNcfOptionsTrainer", "finetune_batches", "fit_pmgt_ncf",
           "check_ncf_model_covered", "ncf_model_grad_host", "ncf_model_layout", "NcfModelGrad", "NcfModelTrainer", "fit_ncf_model",
           "ncf_model_scores_host", "NcfModelScorer", "dcn_scores_host", "DcnScorer", "evaluate_catalogue", "heldout_ranks_host",
           "catalogue_metrics_host", "heldout_csr", "HeldoutRanks", "CatalogueMetrics", "sgd_step_host", "pair_schedule_steps",
           "ItemGraph", "build_item_graph", "item_graph_host", "synthetic_interactions",
           "ItemSimScorer", "edges_csr", "evaluate_neighbours", "holdout_edges", "item_sim_host", "similar_items",
           "HistoryScorer", "evaluate_history", "history_scores_host", "recommend_from_history",
           "ItemKnnIndex", "ItemKnnScorer", "build_item_knn", "decay_weights", "evaluate_item_knn", "item_knn_scores_host",
           "recommend_item_knn", "weighted_history_csr"]
