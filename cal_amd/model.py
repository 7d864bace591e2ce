"""CausalGCN / CausalGAT / CausalGIN with the reference's nn.Module surface
(model.py:12-450): same constructor arguments (``args`` namespace with
``layers, hidden, with_random, without_node_attention,
without_edge_attention, fc_num, cat_or_add``), same sub-module / state-dict
names, same ``forward(data, eval_random=True) -> (xc_logis, xo_logis,
xco_logis)`` log-probabilities, so ``opts.get_model`` (opts.py:85-119) and the
loops in train_causal.py work unchanged.

The graph operators run on libcalhip through ``cal_amd.ops``; one GraphPlan is
built per batch and shared by every layer.
"""
from __future__ import annotations

import os
import random
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import BatchNorm1d, Linear, ReLU, Sequential

from . import ops
from .gat_conv import GATConv
from .gcn_conv import GCNConv
from .plan import plan_of


class _CausalBase(torch.nn.Module):
    """Everything after the backbone: soft masks, causal/trivial convs, pooling,
    three readouts (model.py:46-75, 97-164)."""

    #: CausalGCN gates the shuffle on args.with_random as well (model.py:149-151);
    #: CausalGAT / CausalGIN do not (model.py:435-436, 298-299).
    _gate_on_with_random = False

    def _build_head(self, hidden, hidden_out, GConv):
        self.edge_att_mlp = nn.Linear(hidden * 2, 2)
        self.node_att_mlp = nn.Linear(hidden, 2)
        self.bnc = BatchNorm1d(hidden)
        self.bno = BatchNorm1d(hidden)
        self.context_convs = GConv(hidden, hidden)
        self.objects_convs = GConv(hidden, hidden)
        # context mlp
        self.fc1_bn_c = BatchNorm1d(hidden)
        self.fc1_c = Linear(hidden, hidden)
        self.fc2_bn_c = BatchNorm1d(hidden)
        self.fc2_c = Linear(hidden, hidden_out)
        # object mlp
        self.fc1_bn_o = BatchNorm1d(hidden)
        self.fc1_o = Linear(hidden, hidden)
        self.fc2_bn_o = BatchNorm1d(hidden)
        self.fc2_o = Linear(hidden, hidden_out)
        # random mlp
        if self.args.cat_or_add == "cat":
            self.fc1_bn_co = BatchNorm1d(hidden * 2)
            self.fc1_co = Linear(hidden * 2, hidden)
        elif self.args.cat_or_add == "add":
            self.fc1_bn_co = BatchNorm1d(hidden)
            self.fc1_co = Linear(hidden, hidden)
        else:
            assert False
        self.fc2_bn_co = BatchNorm1d(hidden)
        self.fc2_co = Linear(hidden, hidden_out)

    def _init_bn(self):
        for m in self.modules():                                   # model.py:80-83
            if isinstance(m, torch.nn.BatchNorm1d):
                torch.nn.init.constant_(m.weight, 1)
                torch.nn.init.constant_(m.bias, 0.0001)

    # -- hooks -----------------------------------------------------------------
    def _backbone(self, x, edge_index, plan, edge_mask=None):
        raise NotImplementedError

    #: CausalGCN / CausalGAT: run forward/backward on the native step engine (cal_amd/csrc/engine.hip)
    #: behind this same nn.Module / autograd surface.  Set False for the operator-level path.
    use_engine = os.environ.get("CAL_AMD_ENGINE", "1") != "0"

    def engine(self):
        """The model's StepEngine (created on first use) when its parameters are on the GPU and the engine covers this
        variant; else ``None``."""
        p0 = next(self.parameters())
        return self._engine_for(p0)

    def _engine_for(self, x):
        from . import engine as eng_mod
        if not (self.use_engine and x.is_cuda and isinstance(self, (CausalGCN, CausalGAT, CausalGIN)) and eng_mod.supported(self)):
            return None
        eng = getattr(self, "_engine", None)
        p0 = next(self.parameters())
        if eng is not None:
            lo = eng.flat_p.data_ptr()
            if not (lo <= p0.data_ptr() < lo + 4 * eng.flat_p.numel()):
                eng = None                                   # parameters were moved (.to/.cuda): rebuild
        if eng is None:
            eng = eng_mod.StepEngine(self)
            object.__setattr__(self, "_engine", eng)
        return eng

    def forward(self, data, eval_random=True, perm=None, _objects_raw=False):
        x = data.x if data.x is not None else data.feat
        # (_objects_raw: CausalGIN's train_type = "irm" also returns the objects head's raw logits -- operator-level path)
        eng = None if _objects_raw else self._engine_for(x)
        if eng is not None:
            from .engine import engine_forward_autograd
            if perm is None:
                perm = eng.perm_stage().put(self.intervention_list(int(data.num_graphs), eval_random))
            else:
                perm = perm.to(x.device) if perm.is_cuda else eng.perm_stage().put(perm)  # (pinned ring: a pageable H2D copy blocks the host)
            if self.training and torch.is_grad_enabled():
                return engine_forward_autograd(eng, data, perm)
            eng.forward(data, perm, training=self.training)
            return eng.logp_copy()
        edge_index = data.edge_index
        plan = plan_of(data)
        x = self.bn_feat(x)
        x = self.conv_feat(x, edge_index, relu=True)
        x = self._backbone(x, edge_index, plan)

        if getattr(self, "without_edge_attention", False):
            edge_att = torch.full((2, plan.E), 0.5, dtype=x.dtype, device=x.device)   # model.py:100
        else:
            edge_att = ops.edge_attention(x, self.edge_att_mlp.weight, self.edge_att_mlp.bias, plan)
        edge_weight_c, edge_weight_o = edge_att[0], edge_att[1]

        if getattr(self, "without_node_attention", False):
            xc = 0.5 * x                                                                # model.py:107-111
            xo = 0.5 * x
        else:
            xc, xo, _ = ops.node_attention_split(x, self.node_att_mlp.weight, self.node_att_mlp.bias)
        xc = self.context_convs(self.bnc(xc), edge_index, edge_weight_c, plan=plan, relu=True)
        xo = self.objects_convs(self.bno(xo), edge_index, edge_weight_o, plan=plan, relu=True)

        xc = ops.add_pool(xc, plan)
        xo = ops.add_pool(xo, plan)

        xc_logis = self.context_readout_layer(xc)
        xo_logis = self.objects_readout_layer(xo, "irm" if _objects_raw else "base")
        xco_logis = self.random_readout_layer(xc, xo, eval_random=eval_random, perm=perm)
        return xc_logis, xo_logis, xco_logis

    def _attention_scores(self, data):
        """Operator-level causal scores (model.py:85-111 up to the soft masks: backbone and attention, no convolutions or
        readouts): edge ``edge_att[:, 1]`` [E] and node ``node_att[:, 1]`` [N], column 1 being the objects branch.  Runs in
        the module's current mode; ``cal_amd.explain`` calls it in eval mode under ``no_grad``."""
        x, plan = self._embed(data)
        if getattr(self, "without_edge_attention", False):
            edge = torch.full((plan.E,), 0.5, dtype=x.dtype, device=x.device)
        else:
            edge = ops.edge_attention(x, self.edge_att_mlp.weight, self.edge_att_mlp.bias, plan)[1]
        if getattr(self, "without_node_attention", False):
            node = torch.full((x.size(0),), 0.5, dtype=x.dtype, device=x.device)
        else:
            node = ops.node_attention_split(x, self.node_att_mlp.weight, self.node_att_mlp.bias)[2][:, 1]
        return edge, node

    def _embed(self, data):
        """Operator-level backbone (model.py:85-95): ``(x [N, H], plan)``, the rows both attention MLPs read.  Runs in the
        module's current mode and grad mode."""
        x = data.x if data.x is not None else data.feat
        edge_index = data.edge_index
        plan = plan_of(data)
        x = self.bn_feat(x)
        x = self.conv_feat(x, edge_index, relu=True)
        return self._backbone(x, edge_index, plan), plan

    def _node_embeddings(self, data):
        """The backbone output ``x`` [N, H] that ``_attention_scores`` feeds to ``edge_att_mlp``, in eval mode under ``no_grad``
        (``model.training`` is put back): the input of ``cal_amd.pgexplain``'s edge MLP."""
        from .explain import _eval_mode
        with _eval_mode(self):
            return self._embed(data)[0]

    def _pooled(self, data):
        """Operator-level forward up to the add-pool (model.py:85-116): the pooled trivial rows ``xc`` [B, H] and objects rows
        ``xo`` [B, H], the inputs of the three readouts.  Runs in the module's current mode; ``cal_amd.intervene`` calls it in
        eval mode under ``no_grad``."""
        x = data.x if data.x is not None else data.feat
        edge_index = data.edge_index
        plan = plan_of(data)
        x = self.bn_feat(x)
        x = self.conv_feat(x, edge_index, relu=True)
        x = self._backbone(x, edge_index, plan)
        if getattr(self, "without_edge_attention", False):
            edge_att = torch.full((2, plan.E), 0.5, dtype=x.dtype, device=x.device)
        else:
            edge_att = ops.edge_attention(x, self.edge_att_mlp.weight, self.edge_att_mlp.bias, plan)
        if getattr(self, "without_node_attention", False):
            xc = 0.5 * x
            xo = 0.5 * x
        else:
            xc, xo, _ = ops.node_attention_split(x, self.node_att_mlp.weight, self.node_att_mlp.bias)
        xc = self.context_convs(self.bnc(xc), edge_index, edge_att[0], plan=plan, relu=True)
        xo = self.objects_convs(self.bno(xo), edge_index, edge_att[1], plan=plan, relu=True)
        return ops.add_pool(xc, plan), ops.add_pool(xo, plan)

    def _masked_forward(self, data, edge_mask=None, node_mask=None):
        """Operator-level soft-mask forward with the identity intervention permutation -> the three
        log-prob heads ``(c, o, co)`` [B, C], differentiable in the masks.  ``edge_mask`` float32 [E] >= 0 weighs every edge
        column through every convolution, backbone included: the GCNConvs take it as (a factor of) ``edge_weight``, GINConv as
        the weight of its sum, GATConv inside its edge softmax; ``conv_feat`` (no propagation), the attention MLPs, the pooling
        and the readouts are as in ``forward``.  ``node_mask`` float32 [N] >= 0 puts ``n_u n_v`` on column (u, v) and scales the
        node's rows just before the add-pool.  A column at 0 is the graph without it, a node at 0 the graph without that node,
        all ones the model as it is.  Meant for eval mode (``cal_amd.gradient`` sets it); a GATConv refuses a mask in training
        mode with dropout."""
        x = data.x if data.x is not None else data.feat
        edge_index = data.edge_index
        plan = plan_of(data)
        m = None
        if edge_mask is not None:
            m = edge_mask.view(-1)
            if m.numel() != plan.E:
                raise ValueError("edge_mask must have one entry per edge column (%d, got %d)" % (plan.E, m.numel()))
        if node_mask is not None:
            node_mask = node_mask.view(-1)
            nm = ops.node_mask_columns(node_mask, plan)
            m = nm if m is None else m * nm
        if m is None:
            m = plan.ones()[1][:plan.E]
        x = self.bn_feat(x)
        x = self.conv_feat(x, edge_index, relu=True)
        x = self._backbone(x, edge_index, plan, m)
        if getattr(self, "without_edge_attention", False):
            edge_weight_c = edge_weight_o = 0.5 * m                                         # model.py:100
        else:
            edge_att = ops.edge_attention(x, self.edge_att_mlp.weight, self.edge_att_mlp.bias, plan)
            edge_weight_c, edge_weight_o = edge_att[0] * m, edge_att[1] * m
        if getattr(self, "without_node_attention", False):
            xc = 0.5 * x
            xo = 0.5 * x
        else:
            xc, xo, _ = ops.node_attention_split(x, self.node_att_mlp.weight, self.node_att_mlp.bias)
        xc = self.context_convs(self.bnc(xc), edge_index, edge_weight_c, plan=plan, relu=True)
        xo = self.objects_convs(self.bno(xo), edge_index, edge_weight_o, plan=plan, relu=True)
        if node_mask is not None:
            xc = xc * node_mask.view(-1, 1)
            xo = xo * node_mask.view(-1, 1)
        xc = ops.add_pool(xc, plan)
        xo = ops.add_pool(xo, plan)
        perm = torch.arange(xc.size(0), device=xc.device)
        return (self.context_readout_layer(xc), self.objects_readout_layer(xo),
                self.random_readout_layer(xc, xo, eval_random=False, perm=perm))

    def saliency(self, data, **kw):
        """``cal_amd.gradient.saliency(self, data, **kw)``: the gradient of ``p(ŷ)`` w.r.t. a soft mask of every edge or node."""
        from .gradient import saliency
        return saliency(self, data, **kw)

    def integrated_gradients(self, data, **kw):
        """``cal_amd.gradient.integrated_gradients(self, data, **kw)``: that gradient integrated from the empty to the full graph."""
        from .gradient import integrated_gradients
        return integrated_gradients(self, data, **kw)

    def learn_mask(self, data, **kw):
        """``cal_amd.maskopt.learn_mask(self, data, **kw)``: a soft mask per graph trained to keep ``p(ŷ)`` while small and binary."""
        from .maskopt import learn_mask
        return learn_mask(self, data, **kw)

    def fit_explainer(self, loader, device, **kw):
        """``cal_amd.pgexplain.fit_explainer(self, loader, device, **kw)``: an edge MLP trained once to explain any graph."""
        from .pgexplain import fit_explainer
        return fit_explainer(self, loader, device, **kw)

    def explain_edges(self, explainer, data, **kw):
        """``cal_amd.pgexplain.explain_edges(self, explainer, data, **kw)``: that MLP's mask of ``data``, two forwards."""
        from .pgexplain import explain_edges
        return explain_edges(self, explainer, data, **kw)

    def intervene(self, data, **kw):
        """``cal_amd.intervene.intervene(self, data, **kw)``: the ``co`` head over every (graph, trivial partner) pair."""
        from .intervene import intervene
        return intervene(self, data, **kw)

    def nearest_examples(self, data, bank, **kw):
        """``cal_amd.neighbors.nearest_examples(self, data, bank, **kw)``: the bank graphs nearest to every graph of the batch in
        the objects or the trivial space."""
        from .neighbors import nearest_examples
        return nearest_examples(self, data, bank, **kw)

    def knn_probe(self, bank, **kw):
        """``cal_amd.neighbors.knn_probe(bank, **kw)``: kNN accuracy of the label and the base type from ``xo`` and from ``xc``
        of an ``EmbeddingBank`` of this model."""
        from .neighbors import knn_probe
        return knn_probe(bank, **kw)

    def discover_concepts(self, loader, device, **kw):
        """``cal_amd.concepts.discover_concepts(self, loader, device, **kw)``: k-means on the node embeddings of a loader."""
        from .concepts import discover_concepts
        return discover_concepts(self, loader, device, **kw)

    def assign_concepts(self, data, concepts):
        """``cal_amd.concepts.assign_concepts(self, data, concepts)``: the concept of every node of a new batch."""
        from .concepts import assign_concepts
        return assign_concepts(self, data, concepts)

    def concept_report(self, concepts, **kw):
        """``cal_amd.concepts.concept_report(concepts, **kw)``: purity, motif share, attention and completeness per concept."""
        from .concepts import concept_report
        return concept_report(concepts, **kw)

    def structure_intervention(self, data, **kw):
        """``cal_amd.splice.structure_intervention(self, data, **kw)``: the model on causal parts spliced with other graphs'
        trivial parts."""
        from .splice import structure_intervention
        return structure_intervention(self, data, **kw)

    def occlusion(self, data, **kw):
        """``cal_amd.occlude.occlusion(self, data, **kw)``: leave-one-out scores of every edge column or node."""
        from .occlude import occlusion
        return occlusion(self, data, **kw)

    def faithfulness(self, data, **kw):
        """``cal_amd.occlude.faithfulness(self, data, **kw)``: the causal scores against the occlusion scores."""
        from .occlude import faithfulness
        return faithfulness(self, data, **kw)

    def shapley(self, data, **kw):
        """``cal_amd.coalition.shapley(self, data, **kw)``: permutation-sampled Shapley values of every edge or node."""
        from .coalition import shapley
        return shapley(self, data, **kw)

    def kernel_shap(self, data, **kw):
        """``cal_amd.surrogate.kernel_shap(self, data, **kw)``: Shapley values from a fixed budget of sampled coalitions."""
        from .surrogate import kernel_shap
        return kernel_shap(self, data, **kw)

    def local_surrogate(self, data, **kw):
        """``cal_amd.surrogate.local_surrogate(self, data, **kw)``: a local linear fit and its weighted R^2."""
        from .surrogate import local_surrogate
        return local_surrogate(self, data, **kw)

    def perturbation_curve(self, data, **kw):
        """``cal_amd.coalition.perturbation_curve(self, data, **kw)``: insertion and deletion curves under a ranking."""
        from .coalition import perturbation_curve
        return perturbation_curve(self, data, **kw)

    def counterfactual(self, data, **kw):
        """``cal_amd.counterfactual.counterfactual(self, data, **kw)``: a small set of edges or nodes whose removal flips the prediction."""
        from .counterfactual import counterfactual
        return counterfactual(self, data, **kw)

    def ranking_flip(self, data, order=None, **kw):
        """``cal_amd.counterfactual.ranking_flip(self, data, order, **kw)``: the smallest flipping prefix of a ranking."""
        from .counterfactual import ranking_flip
        return ranking_flip(self, data, order, **kw)

    def noise_curve(self, data, **kw):
        """``cal_amd.noise.noise_curve(self, data, **kw)``: the prediction under growing random edge insertion / deletion."""
        from .noise import noise_curve
        return noise_curve(self, data, **kw)

    def stability(self, data, **kw):
        """``cal_amd.noise.stability(self, data, **kw)``: the causal edge ranking on noisy replicas against the clean graph's."""
        from .noise import stability
        return stability(self, data, **kw)

    def explanation_census(self, data, **kw):
        """``cal_amd.wl.explanation_census(self, data, **kw)``: the WL shape of every graph's causal explanation."""
        from .wl import explanation_census
        return explanation_census(self, data, **kw)

    def explanation_motifs(self, data, **kw):
        """``cal_amd.motif.explanation_motifs(self, data, **kw)``: the prototypes every graph's causal explanation contains or is."""
        from .motif import explanation_motifs
        return explanation_motifs(self, data, **kw)

    def structural_baseline(self, data, **kw):
        """``cal_amd.centrality.structural_baseline(self, data, **kw)``: the causal attention against structure-only rankings."""
        from .centrality import structural_baseline
        return structural_baseline(self, data, **kw)

    def explanation_locality(self, data, **kw):
        """``cal_amd.centrality.explanation_locality(self, data, **kw)``: how far from the motif the explanation's edges lie."""
        from .centrality import explanation_locality
        return explanation_locality(self, data, **kw)

    def explain(self, data, **kw):
        """``cal_amd.explain.explain(self, data, **kw)``: per-graph top-k causal subgraphs of ``data``."""
        from .explain import explain
        return explain(self, data, **kw)

    def context_readout_layer(self, x):
        x = self.fc1_bn_c(x)
        x = ops.linear(x, self.fc1_c.weight, self.fc1_c.bias, relu=True)     # Linear + ReLU on the MFMA GEMM
        x = self.fc2_bn_c(x)
        x = ops.linear(x, self.fc2_c.weight, self.fc2_c.bias)
        return F.log_softmax(x, dim=-1)

    def objects_readout_layer(self, x, train_type="base"):
        """model.py:136-143; CausalGIN's variant (model.py:281-292) also hands back the raw logits for train_type = "irm"."""
        x = self.fc1_bn_o(x)
        x = ops.linear(x, self.fc1_o.weight, self.fc1_o.bias, relu=True)     # Linear + ReLU on the MFMA GEMM
        x = self.fc2_bn_o(x)
        x = ops.linear(x, self.fc2_o.weight, self.fc2_o.bias)
        if train_type == "irm":
            return x, F.log_softmax(x, dim=-1)
        return F.log_softmax(x, dim=-1)

    def intervention_list(self, num, eval_random):
        """model.py:147-152: Python ``random.shuffle`` of range(num), gated as the reference gates it (the list itself)."""
        l = [i for i in range(num)]
        gate = eval_random and (self.with_random if self._gate_on_with_random else True)
        if gate:
            random.shuffle(l)
        return l

    def intervention_index(self, num, eval_random):
        return torch.tensor(self.intervention_list(num, eval_random))

    def random_readout_layer(self, xc, xo, eval_random, perm=None):
        num = xc.shape[0]
        random_idx = self.intervention_index(num, eval_random) if perm is None else perm
        random_idx = random_idx.to(xc.device)
        if self.args.cat_or_add == "cat":
            x = torch.cat((xc[random_idx], xo), dim=1)
        else:
            x = xc[random_idx] + xo
        x = self.fc1_bn_co(x)
        x = ops.linear(x, self.fc1_co.weight, self.fc1_co.bias, relu=True)     # Linear + ReLU on the MFMA GEMM
        x = self.fc2_bn_co(x)
        x = ops.linear(x, self.fc2_co.weight, self.fc2_co.bias)
        return F.log_softmax(x, dim=-1)


class CausalGCN(_CausalBase):
    """model.py:12-164."""
    _gate_on_with_random = True

    def __init__(self, num_features, num_classes, args, gfn=False, collapse=False, residual=False,
                 res_branch="BNConvReLU", global_pool="sum", dropout=0, edge_norm=True):
        super().__init__()
        num_conv_layers = args.layers
        hidden = args.hidden
        self.args = args
        self.dropout = dropout
        self.with_random = args.with_random
        self.without_node_attention = args.without_node_attention
        self.without_edge_attention = args.without_edge_attention
        GConv = partial(GCNConv, edge_norm=edge_norm, gfn=gfn)
        self.num_classes = num_classes
        self.fc_num = args.fc_num
        self.bn_feat = BatchNorm1d(num_features)
        self.conv_feat = GCNConv(num_features, hidden, gfn=True)
        self.bns_conv = torch.nn.ModuleList()
        self.convs = torch.nn.ModuleList()
        for _ in range(num_conv_layers):
            self.bns_conv.append(BatchNorm1d(hidden))
            self.convs.append(GConv(hidden, hidden))
        self._build_head(hidden, num_classes, GConv)
        self._init_bn()

    def _backbone(self, x, edge_index, plan, edge_mask=None):
        for i, conv in enumerate(self.convs):                     # model.py:93-95
            x = self.bns_conv[i](x)
            x = conv(x, edge_index, edge_mask, plan=plan, relu=True)
        return x


class CausalGAT(_CausalBase):
    """model.py:315-450."""

    def __init__(self, num_features, num_classes, args, head=4, dropout=0.2):
        super().__init__()
        num_conv_layers = args.layers
        hidden = args.hidden
        self.args = args
        self.dropout = dropout
        self.with_random = getattr(args, "with_random", True)
        GConv = partial(GCNConv, edge_norm=True, gfn=False)
        self.num_classes = num_classes
        self.fc_num = args.fc_num
        self.bn_feat = BatchNorm1d(num_features)
        self.conv_feat = GCNConv(num_features, hidden, gfn=True)
        self.bns_conv = torch.nn.ModuleList()
        self.convs = torch.nn.ModuleList()
        for _ in range(num_conv_layers):
            self.bns_conv.append(BatchNorm1d(hidden))
            self.convs.append(GATConv(hidden, int(hidden / head), heads=head, dropout=dropout))
        self._build_head(hidden, num_classes, GConv)
        self._init_bn()

    def _backbone(self, x, edge_index, plan, edge_mask=None):
        for i, conv in enumerate(self.convs):                     # model.py:388-390
            x = self.bns_conv[i](x)
            x = conv(x, edge_index, plan=plan, relu=True, edge_mask=edge_mask)
        return x


class GINConv(torch.nn.Module):
    """PyG GINConv(nn): nn((1 + eps) * x + sum_j x_j), eps = 0 fixed (model.py:188)."""

    def __init__(self, nn_module, eps=0.0):
        super().__init__()
        self.nn = nn_module
        self.initial_eps = float(eps)
        self.register_buffer("eps", torch.tensor([float(eps)]))     # PyG keeps eps in the state dict

    def forward(self, x, edge_index, *, plan=None, edge_mask=None):
        from .plan import GraphPlan
        if plan is None:
            plan = GraphPlan(edge_index, x.size(0))
        out = ops.gin_aggregate(x, plan, self.initial_eps, edge_weight=edge_mask)
        lin1, bn, _, lin2, _ = self.nn                               # model.py:189-194
        out = ops.linear(out, lin1.weight, lin1.bias)
        out = torch.relu(bn(out))
        return ops.linear(out, lin2.weight, lin2.bias, relu=True)


class CausalGIN(_CausalBase):
    """model.py:166-313 (SURVEY.md section 8f "next")."""

    def __init__(self, num_features, num_classes, args, gfn=False, edge_norm=True):
        super().__init__()
        hidden = args.hidden
        self.args = args
        self.with_random = getattr(args, "with_random", True)
        GConv = partial(GCNConv, edge_norm=edge_norm, gfn=gfn)
        self.num_classes = num_classes
        self.fc_num = args.fc_num
        self.bn_feat = BatchNorm1d(num_features)
        self.conv_feat = GCNConv(num_features, hidden, gfn=True)
        self.bns_conv = torch.nn.ModuleList()
        self.convs = torch.nn.ModuleList()
        for _ in range(args.layers):
            self.convs.append(GINConv(Sequential(Linear(hidden, hidden), BatchNorm1d(hidden), ReLU(),
                                                 Linear(hidden, hidden), ReLU())))
        self._build_head(hidden, num_classes, GConv)
        self._init_bn()

    def _backbone(self, x, edge_index, plan, edge_mask=None):
        for conv in self.convs:                                   # model.py:244-245
            x = conv(x, edge_index, plan=plan, edge_mask=edge_mask)
        return x

    def forward(self, data, eval_random=True, train_type="base", perm=None):
        """model.py:234-264: ``forward(data, eval_random=True, train_type="base")``.  ``train_type="irm"`` makes the objects
        head return ``(raw logits, log-probs)`` instead of the log-probs (model.py:281-292) -- dead in the reference's own loops
        (train_causal.py:177,212 never pass it) but part of the module surface; that variant runs on the operator-level path,
        where the raw logits are differentiable."""
        if torch.is_tensor(train_type):                               # (a caller of the base-class order: forward(data, eval_random, perm))
            perm, train_type = train_type, "base"
        return super().forward(data, eval_random, perm=perm, _objects_raw=(train_type == "irm"))
