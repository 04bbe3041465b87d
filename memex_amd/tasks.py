"""The two callers of the hot path, as far as the path goes (no SQL, no HTTP): what the worker does with a document and what
the API does with a query.

=================================  ==========================================================================
reference                          here
=================================  ==========================================================================
``process_embeddings``             :func:`process_embeddings` -- embed the document's windows, name every segment
(lib/worker/src/tasks.rs:9-66)     ``v5(NAMESPACE, "{doc_uuid}-{idx}")`` with ``doc_uuid = v5(NAMESPACE, task_id)``
                                   (db/document.rs:73-74), hand them to ``add_vectors``; returns the ``VectorData`` the
                                   reference also writes to its ``embeddings`` table
``handle_search_docs``             :func:`search_docs` -- ``encode_single(query)`` -> ``search(vector, limit)`` ->
(lib/api/.../handlers.rs:55-109)   ``(segment _id, score)`` pairs (the handler then looks each _id up in SQL)
=================================  ==========================================================================

:func:`search_docs_multi` has no counterpart in the reference: several texts for one request (the phrasings of a question, a question
and a hypothetical answer, the last turns of a conversation), one ranked list back (``search_fused``).

:func:`search_docs_feedback` has none either: a query (or none) together with the segments marked relevant and irrelevant, one list back
(``search_like``, Rocchio relevance feedback computed on the device).

:func:`rerank_docs` has none either: a query and the segments something else found (a keyword backend, a cached result page, the
caller's own working set), those segments back with their exact scores, best first (``rerank``; nothing is searched).

:func:`search_documents` has none either: ``search_docs`` returns segments despite its name, and so does the reference's handler; this
one returns the best DOCUMENTS, each by its best segment (``search_documents`` of the store, over a grouping that
:func:`group_document` fills from a ``process_embeddings`` result).

:func:`search_document_passages` and :func:`search_docs_spread` go one step further: the best documents with their few best segments
each, and a flat list in which no document supplies more than a few segments -- what a caller that assembles context asks for.

:func:`search_docs_recent` has none either: relevance plus recency.  :func:`stamp_document` stores ``exp2((t - t0) / half_life)`` for
a document's segments once, at ingest; a query at time ``now`` multiplies its weight by ``exp2(-(now - t0) / half_life)``, so the
boost a segment gets is ``weight * exp2(-(now - t) / half_life)`` and the resident values are never rewritten as time passes.

The ids are the reference's own (RFC 4122 v5 over the same namespace), so a collection filled through this mirror lines up
with the rows a memex worker would have written for the same task ids.
"""
from __future__ import annotations

import uuid
from typing import List, Sequence, Tuple

import numpy as np

from .storage import VectorData

NAMESPACE = uuid.UUID("5fdfe40a-de2c-11ed-bfa7-00155deae876")   # lib/libmemex/src/lib.rs:6


def document_uuid(task_id: int) -> str:
    """db/document.rs:74: ``Uuid::new_v5(&NAMESPACE, task.id.to_string().as_bytes())``."""
    return str(uuid.uuid5(NAMESPACE, str(task_id)))


def segment_uuid(doc_uuid: str, idx: int) -> str:
    """tasks.rs:36-40: ``Uuid::new_v5(&NAMESPACE, format!("{doc_uuid}-{idx}").as_bytes())``."""
    return str(uuid.uuid5(NAMESPACE, f"{doc_uuid}-{idx}"))


def process_embeddings(client, embedder, task_id: int, content: str) -> List[VectorData]:
    """tasks.rs:9-66 without the SQL: ``embedder.encode(content)`` -> one ``VectorData`` per window -> ``client.add_vectors``.
    Like the reference, a failing ``add_vectors`` is the caller's to log (the exception propagates here)."""
    embeddings = embedder.encode(content)                                  # :19
    doc = document_uuid(task_id)                                           # :28 (document::ActiveModel::from_task)
    vectors = [VectorData(_id=segment_uuid(doc, idx), document_id=doc, text=e.content, vector=e.vector, segment_id=idx)
               for idx, e in enumerate(embeddings)]                        # :34-56
    client.add_vectors(vectors)                                            # :59
    return vectors


def search_docs(client, embedder, query: str, limit: int = 10) -> List[Tuple[str, float]]:
    """handlers.rs:72-85: embed the query, search; ``ValueError("Invalid query")`` where the handler rejects (:74-78)."""
    res = embedder.encode_single(query)
    if res is None:
        raise ValueError("Invalid query")
    return client.search(res.vector, limit)


def search_docs_multi(client, embedder, queries: Sequence[str], limit: int = 10, mode: str = "max") -> List[Tuple[str, float]]:
    """``search_docs`` for several texts at once: each is embedded with ``encode_single`` (the embedder's actor batches what is
    queued), the vectors go to ``client.search_fused`` and ONE list of ``(segment _id, score)`` pairs comes back -- ``mode="max"``:
    the best score over the texts, ``"rrf"``: reciprocal-rank fusion.  ``ValueError("Invalid query")`` if any text embeds to nothing
    (or none is given)."""
    vectors = []
    for text in queries:
        res = embedder.encode_single(text)
        if res is None:
            raise ValueError("Invalid query")
        vectors.append(res.vector)
    if not vectors:
        raise ValueError("Invalid query")
    return client.search_fused(vectors, limit, mode)


def search_docs_feedback(client, embedder, query, relevant: Sequence[str], irrelevant: Sequence[str] = (),
                         limit: int = 10) -> List[Tuple[str, float]]:
    """``search_docs`` with relevance feedback: the segments the user (or the agent) marked ``relevant`` pull the query towards them,
    the ``irrelevant`` ones push it away (``client.search_like``, Rocchio weights), and the marked segments are not listed again.
    ``query`` may be ``None``: more like the relevant segments alone.  ``ValueError("Invalid query")`` where ``search_docs`` raises
    it: a query that embeds to nothing."""
    vec = None
    if query is not None:
        res = embedder.encode_single(query)
        if res is None:
            raise ValueError("Invalid query")
        vec = res.vector
    return client.search_like(list(relevant), list(irrelevant), limit, vec)


def group_document(grouping, vectors: Sequence[VectorData]) -> None:
    """Tell a grouping (``HipFlatStore.make_grouping``) which document the segments of a ``process_embeddings`` result belong to:
    every ``VectorData`` goes under its ``document_id``.  Call it after the vectors were added."""
    by_doc = {}
    for v in vectors:
        by_doc.setdefault(v.document_id, []).append(v._id)
    for doc, ids in by_doc.items():
        grouping.assign(doc, ids)


def search_documents(client, embedder, grouping, query: str, limit: int = 10):
    """``search_docs`` that answers in DOCUMENTS: ``encode_single(query)`` -> ``client.search_documents(vector, limit, grouping)`` ->
    ``(hits, complete)``, each hit ``(document id or None, best segment _id, score, group_rows)`` -- the ``limit`` best documents,
    each represented by its best segment, where ``search_docs`` may return ``limit`` windows of one document.
    ``ValueError("Invalid query")`` where ``search_docs`` raises it."""
    res = embedder.encode_single(query)
    if res is None:
        raise ValueError("Invalid query")
    return client.search_documents(res.vector, limit, grouping)


def search_document_passages(client, embedder, grouping, query: str, limit: int = 10, passages: int = 3):
    """``search_documents`` with context to assemble: ``client.search_document_passages(vector, limit, grouping, passages)`` ->
    ``(hits, complete)``, each hit ``(document id or None, [(segment _id, score), ...], members_complete)`` -- the ``limit`` best
    documents, each with its ``passages`` best segments.  ``ValueError("Invalid query")`` where ``search_docs`` raises it."""
    res = embedder.encode_single(query)
    if res is None:
        raise ValueError("Invalid query")
    return client.search_document_passages(res.vector, limit, grouping, passages)


def search_docs_spread(client, embedder, grouping, query: str, limit: int = 10, per_document: int = 2):
    """``search_docs`` in which no document supplies more than ``per_document`` segments: ``client.search_spread(vector, limit,
    grouping, per_document)`` -> ``(hits, complete)``, each hit ``(document id or None, segment _id, score)``, a flat list best
    first.  ``ValueError("Invalid query")`` where ``search_docs`` raises it."""
    res = embedder.encode_single(query)
    if res is None:
        raise ValueError("Invalid query")
    return client.search_spread(res.vector, limit, grouping, per_document)


def stamp_document(prior, vectors: Sequence[VectorData], t: float, half_life: float, t0: float) -> None:
    """Ingest side of :func:`search_docs_recent`: the segments of a ``process_embeddings`` result, written at time ``t``, get the
    prior ``exp2((t - t0) / half_life)`` (``StorePrior.set_document``).  Call it after the vectors were added.  The value is an f32:
    it overflows about 127 half-lives after ``t0`` (``ValueError``), and a query's folded weight underflows about as far out, so
    after roughly 120 half-lives ``t0`` must be moved and the values written again."""
    value = _stamp_value(t, half_life, t0)
    ids = [v._id for v in vectors]
    if ids:
        prior.set_document(ids, value)


def _stamp_value(t: float, half_life: float, t0: float) -> float:
    """The f32 prior of a segment written at ``t``: ``exp2((t - t0) / half_life)``; ``ValueError`` when it overflows."""
    with np.errstate(over="ignore"):
        value = float(np.float32(np.exp2((np.float64(t) - np.float64(t0)) / np.float64(half_life))))
    if not np.isfinite(value):
        raise ValueError("t is too far from t0 for an f32 prior: move t0 and stamp the documents again")
    return value


def recency_weight(weight: float, now: float, half_life: float, t0: float) -> float:
    """The weight a query at time ``now`` carries: ``weight * exp2(-(now - t0) / half_life)``, as an f32."""
    return float(np.float32(np.float64(weight) * np.exp2(-(np.float64(now) - np.float64(t0)) / np.float64(half_life))))


def search_docs_recent(client, embedder, prior, query: str, limit: int = 10, now: float = 0.0, half_life: float = 1.0, t0: float = 0.0,
                       weight: float = 1.0):
    """``search_docs`` that prefers recent segments: ``encode_single(query)`` -> ``client.search_boosted(vector, limit, prior,
    recency_weight(weight, now, half_life, t0))`` -> ``(hits, complete)``, each hit ``(segment _id, score, prior, combined)``.  With
    the priors of :func:`stamp_document` a segment written at ``t`` is ranked by ``score + weight * exp2(-(now - t) / half_life)``:
    ``weight`` is the boost of a segment written this instant, halved every ``half_life``.  ``ValueError("Invalid query")`` where
    ``search_docs`` raises it."""
    res = embedder.encode_single(query)
    if res is None:
        raise ValueError("Invalid query")
    return client.search_boosted(res.vector, limit, prior, recency_weight(weight, now, half_life, t0))


def search_docs_since(client, embedder, prior, flt, query: str, limit: int = 10, t_min: float = 0.0, half_life: float = 1.0,
                      t0: float = 0.0, now: float = 0.0, weight: float = 0.0):
    """``search_docs`` over the segments stamped at or after ``t_min`` only: ``flt.allow_where(prior, lo=v)`` with ``v`` the value
    :func:`stamp_document` stores for ``t_min`` -- the device picks the rows out of the prior, no id list is built on the host -- then
    ``encode_single(query)`` -> ``client.search_boosted(vector, limit, prior, recency_weight(weight, now, half_life, t0), None, flt)``
    -> ``(hits, complete)`` as :func:`search_docs_recent`.  ``flt`` is a filter of the store (``HipFlatStore.make_filter()``), empty
    or already allowing other rows: the recent segments are added to it, and it can serve later queries with the same ``t_min``
    through ``search_boosted`` directly.  The stored values rise with ``t`` and f32 rounding keeps the order, so a segment stamped at
    ``t >= t_min`` is in the set; segments nobody stamped read 0 and are not.  ``weight = 0`` (the default) ranks by relevance alone.
    ``ValueError("Invalid query")`` where ``search_docs`` raises it."""
    res = embedder.encode_single(query)
    if res is None:
        raise ValueError("Invalid query")
    flt.allow_where(prior, lo=_stamp_value(t_min, half_life, t0))
    return client.search_boosted(res.vector, limit, prior, recency_weight(weight, now, half_life, t0), None, flt)


def rerank_docs(client, embedder, query: str, candidates: Sequence[str], limit: int = 10) -> List[Tuple[str, float]]:
    """Score the ``candidates`` (segment ``_id``s from a keyword backend, a cached page, a working set) against the query and rank
    them: ``encode_single(query)`` -> ``client.rerank(vector, candidates, limit)`` -> ``(segment _id, score)`` pairs, best first,
    with the scores ``search_docs`` would report for them.  ``ValueError("Invalid query")`` where ``search_docs`` raises it."""
    res = embedder.encode_single(query)
    if res is None:
        raise ValueError("Invalid query")
    return client.rerank(res.vector, list(candidates), limit)
