"""mfcd — host side of the MI355X triplet-comparison matrix-factorisation hot path.

`_lib`     ctypes binding of libmfcd_hip.so (C-ABI in include/mfcd.h); raises if it is not built.
`batching` DataLoader -> packed records + per-epoch order, RNG-stream compatible with the reference.
`engine`   fused training epochs / evaluation on the device, in place on the caller's model + Adam.
`metrics`  dense UV^T reconstruction / alignment metrics from the MFMA pass.
`topk`     the k best / worst columns of rows of a dense or factored score matrix (mfcd_topk_rows).
`pairs`    exact all-pairs BTL risk, pairwise accuracy and Kendall counts per row (mfcd_pair_stats_rows).
`foldin`   the exact block steps: one Newton solve per user with V fixed (mfcd_fold_in_users), one per item with U and
           the other items fixed (mfcd_item_step).
`alternating` the two block steps alternated: monotone exact-block descent of the regularised BTL objective.
`newton`   both tables at once: gradient and Hessian-vector product of the sampled objective (mfcd_triplet_rows) and a
           trust-region Newton-CG fit on them.
`population` the exact block steps of the ridge-regularised population risk: Newton-CG on mfcd_pair_hvp_rows.
`ratings`  the all-pairs risk, gradient and metrics on observed ratings: ragged rows (mfcd_pair_ragged_stats, _grad).
`ratings_exact` the exact block steps of the ridge-regularised ratings risk: Newton-CG on mfcd_pair_ragged_hvp.
`ranking` ranks of held-out entries among all admissible items and the full-catalogue ranking metrics (mfcd_rank_entries).
`implicit` the exact observed-versus-unobserved logistic risk on implicit feedback, its fit and metrics (mfcd_implicit_rows).
`implicit_exact` the exact block steps of the ridge-regularised implicit risk: Newton-CG on mfcd_implicit_hvp_rows.
`design`   the D-optimal comparison design of every user: pairwise Frank-Wolfe on the arg-max of mfcd_pair_best_rows.
"""
from . import (_lib, alternating, batching, design, engine, foldin, implicit, implicit_exact, metrics, newton,  # noqa: F401
               pairs, population, ranking, ratings, ratings_exact, topk)

__all__ = ["_lib", "alternating", "batching", "design", "engine", "foldin", "implicit", "implicit_exact", "metrics", "newton", "pairs",
           "population", "ranking", "ratings", "ratings_exact", "topk"]
