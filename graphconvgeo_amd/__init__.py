"""graphconvgeo_amd -- MI355X-native graph-convolution hot path of afcarl/graphconvgeo.

Product modules (all compute runs in libgcg_spmm.so HIP kernels; no CPU fallback):
  sparse       DeviceCSR (H / X resident in HBM), spmm (= S.dot + fused epilogue)
  layers       GraphConvLayer, SparseConvolutionDenseLayer, ConvolutionDenseLayer, GCN
  ops          the hot path as torch.ops.gcg.* custom ops with fake kernels (torch.compile)
  dense        output layer on the MFMA cores: f32 GEMMs, fused projection + softmax + CE
  distributed  1-D row partition of H + RCCL all-gather / halo exchange of the dense operand
  dist_train   the row-partitioned GCN training step (backward through H's symmetry)
  graph        H = D^-1/2 (A+I) D^-1/2 construction, host (scipy) and device (HIP)
  mentions     mention-graph parsing (host) and projection (HIP), data.py:226-375
  training     what the trainers share: the optimiser base, the epoch loop and its improvement
               rules, the host half of a mini-batch epoch
  mlpconv      MLPCONV trainer (mlpconv.py:121-352) on the GPU
  mlp          MLP mini-batch trainer (mlp.py:96-311) on the GPU, input_convolution (H * X)
  geo          k-d-tree region labels (kdtree.py), class medians, haversine, nearest class and
               geo_eval (mean / median km, Acc@161) on the GPU, data.py:399-419
  mdn          the mixture-density location head (lang2loc.py): fused NLL + gradient, the
               "mixture" prediction rule, NNModel_lang2loc (text -> lat/lon) on the GPU
  loc2lang     the location-to-language model (loc2lang.py): the Gaussian layer, softmax
               cross-entropy against sparse soft targets, Adamax, NNModel_loc2lang (lat/lon -> words)
               and its analyses on the device (local words, word maps, top words, dialect ranking)
  kmeans       get_cluster_centers: k-means++ / Lloyd k-means and the per-cluster statistics that
               start the mixture models' Gaussians, float64 on the GPU
  dialect      the dialect-embedding evaluation (main.py:108-162, 230-281, 364-384): min-max + l1
               scaling, the rank of every gold word among all V neighbours, recall@k, kneighbors
  tfidf        DataLoader.tfidf (data.py:378-397): tokenising on the host or, opt-in, on the GPU
               (tokenize_corpus_device), counting, document frequencies, pruning and tf-idf
               weighting on the GPU, dataloader_features
  grid         grid_representation (loc2lang.py:298-322): coordinates as l1-normalised sparse rows
               over a lat/lon grid, the input of loc2lang's no-MDN baseline
  synth        seeded synthetic graphs / features for the BASELINE configs

`MLP`, `input_convolution`, `NNModel_lang2loc`, `NNModel_lang2locshared`, `NNModel_loc2lang`,
`NNModel_loc2lang_nomdn`, `grid_representation`, `LatLonGrid`, `US_BBOX`, `WORLD_BBOX` and
`DeviceCSR` are imported lazily from the package itself.
"""
import os as _os

__version__ = "0.1.0"

# A captured training step (mlpconv use_graph) has parallel branches: the side-stream weight and
# bias gradients beside the main-stream chain. The HIP runtime replays such branches on this many
# streams (read once, when HIP initialises -- hence here, before any torch.cuda call). Its default
# serialises the branches and the graph ran 2-4 % behind eager; with 8 the World step replays at
# eager's speed (profiles/r06/graph_queues_ab*.txt, tools/gpu/graph_queues.sh). Eager launches
# are unaffected; an explicit setting wins.
_os.environ.setdefault("DEBUG_HIP_FORCE_GRAPH_QUEUES", "8")

__all__ = ["sparse", "ops", "layers", "dense", "distributed", "dist_train", "graph", "mentions",
           "training", "mlpconv", "mlp", "geo", "mdn", "loc2lang", "dialect", "tfidf",
           "grid", "synth", "MLP", "NNModel_loc2lang_nomdn", "grid_representation", "LatLonGrid",
           "US_BBOX", "WORLD_BBOX",
           "input_convolution",
           "NNModel_lang2loc", "NNModel_lang2locshared", "NNModel_loc2lang", "DeviceCSR"]

_LAZY = {"MLP": "mlp", "input_convolution": "mlp", "NNModel_lang2loc": "mdn",
         "NNModel_lang2locshared": "mdn", "NNModel_loc2lang": "loc2lang", "DeviceCSR": "sparse",
         "NNModel_loc2lang_nomdn": "loc2lang", "grid_representation": "grid", "LatLonGrid": "grid",
         "US_BBOX": "grid", "WORLD_BBOX": "grid"}


def __getattr__(name):
    if name in _LAZY:
        import importlib

        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
