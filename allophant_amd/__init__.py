"""allophant_amd: MI355X-native acoustic-encoder forward path for kgnlp/allophant's ``Estimator.predict``.

Hand-written HIP kernels for gfx950 behind a C ABI (``include/allophant_amx.h``), wrapped by a Python façade that keeps
the reference's ``Estimator`` / ``Batch`` / ``Predictions`` names and shapes.  There is no CPU fallback: using the
compute path without the built ``liballophant_amx.so`` raises.
"""
from . import spec, synthetic  # noqa: F401

__all__ = ["spec", "synthetic", "Estimator", "Batch", "Predictions", "GreedyCTCDecoder", "CTCHypothesis", "BeamCTCDecoder",
           "BeamDecoded", "feature_decoders", "EditStatistics", "EvaluationResults", "MultilingualEvaluationResults", "Evaluator",
           "levensthein_statistics", "levensthein_statistics_batch", "Action", "UtteranceEdits", "levensthein_operations",
           "levensthein_operations_batch", "levensthein_substitutions", "to_substitutions", "PropertyWeighting",
           "levensthein_matrix", "levensthein_confusions_batch", "ConfusionCounts", "ConfusionTable", "Alignment", "Aligned", "ctc_forced_align", "label_targets", "segments", "Score", "Scored",
           "Rescored", "ctc_score", "Found", "Hit", "ctc_search", "pick_hits", "query_targets", "LongPlan", "plan_windows",
           "gather_windows", "stitch_windows", "Variants", "Alternatives", "ctc_variants", "PhonotacticLM",
           "TargetGraph", "GraphAlignment", "GraphAligned", "ctc_graph_align", "slot_targets"]
__version__ = "0.1.0"


def __getattr__(name):
    # the façade classes live in .estimator; resolved on first use so that importing the package stays light
    if name in ("Estimator", "Batch", "Predictions", "GreedyCTCDecoder", "CTCHypothesis", "BeamCTCDecoder", "BeamDecoded",
                "feature_decoders"):
        from . import estimator

        return getattr(estimator, name)
    if name in ("EditStatistics", "EvaluationResults", "MultilingualEvaluationResults", "Evaluator", "levensthein_statistics",
                "levensthein_statistics_batch", "Action", "UtteranceEdits", "levensthein_operations", "levensthein_operations_batch",
                "levensthein_substitutions", "to_substitutions", "PropertyWeighting", "levensthein_matrix",
                "levensthein_confusions_batch", "ConfusionCounts", "ConfusionTable"):
        from . import evaluation

        return getattr(evaluation, name)
    if name in ("Alignment", "Aligned", "ctc_forced_align", "label_targets", "segments"):
        from . import alignment

        return getattr(alignment, name)
    if name in ("Score", "Scored", "Rescored", "ctc_score"):
        from . import scoring

        return getattr(scoring, name)
    if name in ("Found", "Hit", "ctc_search", "pick_hits", "query_targets"):
        from . import search

        return getattr(search, name)
    if name in ("LongPlan", "plan_windows", "gather_windows", "stitch_windows"):
        from . import longform

        return getattr(longform, name)
    if name in ("Variants", "Alternatives", "ctc_variants"):
        from . import variants

        return getattr(variants, name)
    if name in ("TargetGraph", "GraphAlignment", "GraphAligned", "ctc_graph_align", "slot_targets"):
        from . import graph_alignment

        return getattr(graph_alignment, name)
    if name == "PhonotacticLM":
        from . import phonotactics

        return phonotactics.PhonotacticLM
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
