"""AddMetadata and its shorthands (reference: nvtabular/ops/add_metadata.py): tags and properties
added to the schema of the selected columns; the data passes through untouched."""
from __future__ import annotations

from ..schema import Tags
from ..selector import ColumnSelector
from .base import Operator


class AddMetadata(Operator):
    accepts_datetime = True

    def __init__(self, tags=None, properties=None):
        super().__init__()
        self.tags = tags or []
        self.properties = properties or {}

    def transform(self, col_selector: ColumnSelector, df):
        return df

    @property
    def output_tags(self):
        return self.tags

    @property
    def output_properties(self):
        return self.properties


class AddTags(AddMetadata):
    def __init__(self, tags=None):
        super().__init__(tags=tags)


class AddProperties(AddMetadata):
    def __init__(self, properties=None):
        super().__init__(properties=properties)


class TagAsUserID(AddTags):
    def __init__(self, tags=None):
        super().__init__(tags=[Tags.ID, Tags.USER])


class TagAsItemID(AddTags):
    def __init__(self, tags=None):
        super().__init__(tags=[Tags.ID, Tags.ITEM])


class TagAsUserFeatures(AddTags):
    def __init__(self, tags=None):
        super().__init__(tags=[Tags.USER])


class TagAsItemFeatures(AddTags):
    def __init__(self, tags=None):
        super().__init__(tags=[Tags.ITEM])
