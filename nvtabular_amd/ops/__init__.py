"""Operator namespace mirroring ``nvtabular.ops`` for the hot path
(nvtabular/ops/__init__.py:21-54): the ops named by the north star plus the
graph-plumbing ops the DSL creates."""
from .add_metadata import (  # noqa: F401
    AddMetadata, AddProperties, AddTags, TagAsItemFeatures, TagAsItemID, TagAsUserFeatures, TagAsUserID)
from .base import Operator, StatOperator  # noqa: F401
from .bucketize import Bucketize  # noqa: F401
from .categorify import Categorify, get_embedding_sizes  # noqa: F401
from .clip_log import Clip, LogOp  # noqa: F401
from .data_stats import DataStats  # noqa: F401
from .difference_lag import DifferenceLag  # noqa: F401
from .drop_low_cardinality import DropLowCardinality  # noqa: F401
from .dropna import Dropna  # noqa: F401
from .fill import FillMedian, FillMissing  # noqa: F401
from .filter import Filter  # noqa: F401
from .groupby import Groupby  # noqa: F401
from .hash_bucket import HashBucket  # noqa: F401
from .hashed_cross import HashedCross  # noqa: F401
from .join_external import JoinExternal  # noqa: F401
from .join_groupby import JoinGroupby  # noqa: F401
from .lambdaop import LambdaOp  # noqa: F401
from .list_slice import ListSlice  # noqa: F401
from .normalize import Normalize, NormalizeMinMax  # noqa: F401
from .reduce_dtype_size import ReduceDtypeSize  # noqa: F401
from .selection import ConcatColumns, Rename, SubsetColumns, SubtractionOp  # noqa: F401
from .target_encoding import TargetEncoding  # noqa: F401
from .value_counts import ValueCount  # noqa: F401
from ..selector import ColumnSelector  # noqa: F401
