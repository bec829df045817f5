"""Mirror of torchreid.metrics (reference torchreid/metrics/{distance,rank,accuracy}.py)."""
from .accuracy import accuracy  # noqa: F401
from .distance import compute_distance_matrix, cosine_distance, euclidean_squared_distance, pair_distances  # noqa: F401
from .rank import eval_cuhk03, eval_market1501, eval_regdb, evaluate_rank  # noqa: F401
from .rank_stream import RankAccumulator, evaluate_rank_streamed, rank_counts_streamed  # noqa: F401
from .search import TopKAccumulator, default_slab_rows, search_topk  # noqa: F401
from .topk import rank_topk  # noqa: F401
