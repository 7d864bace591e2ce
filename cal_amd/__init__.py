"""cal_amd -- MI355X-native (gfx950) implementation of the CAL causal-attention
message-passing hot path (yongduosui/CAL: gcn_conv.py, model.py,
train_causal.py).  Hand-written HIP kernels behind a C ABI
(include/cal_hip.h, cal_amd/csrc) with a thin Python host that keeps the
reference's nn.Module surface.  There is no CPU fallback: compute entry points
raise if libcalhip.so or a GPU is missing."""
__version__ = "0.1.0"

_MASKOPT = ("LearnedMask", "MaskOptimizer", "learn_mask", "mask_agreement")
_PGEXPLAIN = ("EdgeExplainer", "ExplainerTrainer", "ParametricMask", "fit_explainer", "explain_edges", "explainer_agreement",
              "eval_explainer")
_MOTIF = ("MotifMatch", "MotifPatterns", "motif_match", "automorphisms", "contains", "isomorphic", "motif_census",
          "explanation_motifs", "eval_explanation_motifs")
_CENTRALITY = ("Centrality", "hop_distance", "structural_scores", "structural_baseline", "eval_structural_baseline",
               "explanation_locality", "eval_explanation_locality")
_COUNTERFACTUAL = ("Counterfactual", "subset_batch", "pack_bits", "unpack_bits", "beam_step", "ranking_flip", "counterfactual_report",
                   "eval_counterfactual")
_NEIGHBORS = ("KnnResult", "EmbeddingBank", "NearestExamples", "knn", "embedding_bank", "nearest_examples", "knn_probe",
              "eval_disentanglement")
_CONCEPTS = ("KMeansResult", "NodeBank", "Concepts", "kmeans", "node_bank", "discover_concepts", "assign_concepts",
             "concept_report", "eval_concepts")
_SURROGATE = ("Surrogate", "surrogate_fit", "kernel_shap", "local_surrogate", "surrogate_agreement", "eval_surrogate")


def __getattr__(name):
    # the learned-mask explanations (cal_amd/maskopt.py), imported on first use: importing the package loads neither torch nor a
    # library
    if name in _MASKOPT:
        from . import maskopt
        return getattr(maskopt, name)
    if name in _PGEXPLAIN:                                    # the parametric edge explainer (cal_amd/pgexplain.py), likewise
        from . import pgexplain
        return getattr(pgexplain, name)
    if name in _MOTIF:                                        # exact motif matching (cal_amd/motif.py), likewise
        from . import motif
        return getattr(motif, name)
    if name in _CENTRALITY:                                   # graph centralities and the structural baselines, likewise
        # (``cal_amd.centrality`` is the module; its function of that name is ``cal_amd.centrality.centrality``)
        from . import centrality
        return getattr(centrality, name)
    if name in _COUNTERFACTUAL:                               # counterfactual explanations, likewise
        # (``cal_amd.counterfactual`` is the module; its function of that name is ``cal_amd.counterfactual.counterfactual``)
        from . import counterfactual
        return getattr(counterfactual, name)
    if name in _NEIGHBORS:                                    # nearest neighbours in embedding space, likewise
        from . import neighbors
        return getattr(neighbors, name)
    if name in _CONCEPTS:                                     # concept discovery (k-means on node embeddings), likewise
        # (``assign`` stays ``cal_amd.concepts.assign``: the name is too plain for the package)
        from . import concepts
        return getattr(concepts, name)
    if name in _SURROGATE:                                    # surrogate attributions (KernelSHAP, a local linear fit), likewise
        from . import surrogate
        return getattr(surrogate, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
