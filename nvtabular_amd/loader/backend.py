"""Schema plumbing of the dataloaders (the reference's ``nvtabular.loader.backend``)."""
from __future__ import annotations

from ..schema import Schema, Tags


def _augment_schema(schema: Schema, cats=None, conts=None, labels=None, padded_cols=None, padded_lengths=None,
                    pad=False, batch_size=0) -> Schema:
    """The schema with the role of every named column added to its tags: TARGET for ``labels``,
    CATEGORICAL for ``cats``, CONTINUOUS for ``conts``.  ``padded_cols`` / ``padded_lengths`` / ``pad``
    record the list handling in the column's properties (this Schema carries no shapes)."""
    labels = [labels] if isinstance(labels, str) else labels
    out = Schema(schema.column_schemas.values())
    for names, tag in ((labels, Tags.TARGET), (cats, Tags.CATEGORICAL), (conts, Tags.CONTINUOUS)):
        for name in names or []:
            if name not in out:
                raise ValueError(f"column '{name}' is not in the dataset's schema {out.column_names}")
            out.column_schemas[name] = out[name].with_tags(tag)
    for name in padded_cols or []:
        props = {"pad": bool(pad)}
        if padded_lengths and name in padded_lengths:
            props["max_length"] = int(padded_lengths[name])
        out.column_schemas[name] = out[name].with_properties(props)
    return out
