"""splitComponents' host side: from the connected components of a labelling (Context.label_components) to instances.  Pure numpy, no
GPU: the components are a few thousand at most, whatever the number of points, and the one pass over the points is a gather."""
import numpy as np

KEEP = ("all", "largest")


def regroup(labels, model_number, comp, first, sizes, minimum_point_number, keep="all"):
    """(new_labels int32 [n], parent int32 [K']): the components (comp [n] with -1 for a point of no component, first [C], sizes [C], as
    pgx_label_components numbers them) of the labelling `labels` [n] with models 0 .. model_number-1, regrouped into K' instances.
    keep="all": every component of at least minimum_point_number points is an instance; keep="largest": of each model only its largest
    component (ties: the smaller `first`), and only if it passes the same size test.  Instances are ordered by (original label
    ascending, size descending, first ascending); parent[j] is the original model of instance j; every other point gets K'."""
    if keep not in KEEP:
        raise ValueError('keep should be "all" or "largest"')
    labels = np.asarray(labels).reshape(-1)
    comp = np.asarray(comp, dtype=np.int64).reshape(-1)
    first = np.asarray(first, dtype=np.int64).reshape(-1)
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    model = labels[first].astype(np.int64)                      # a component's model is that of any member
    if len(model) and (model.min() < 0 or model.max() >= model_number):
        raise ValueError("a component of a label outside 0 .. model_number-1")
    order = np.lexsort((first, -sizes, model))                  # by (model, size descending, first)
    if keep == "largest":
        head = np.ones(len(order), dtype=bool)
        head[1:] = model[order[1:]] != model[order[:-1]]        # the first of each model's run is its largest, ties to the smaller first
        order = order[head]
    order = order[sizes[order] >= minimum_point_number]
    k = len(order)
    instance = np.full(len(first) + 1, k, dtype=np.int32)       # the last entry serves comp == -1
    instance[order] = np.arange(k, dtype=np.int32)
    return instance[comp], model[order].astype(np.int32)
