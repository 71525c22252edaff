"""pcdet/utils/spconv_utils.py of the reference over this project's own sparse conv classes (pcp_amd/spconv.py)."""
from pcp_amd import spconv


def find_all_spconv_keys(model, prefix=''):
    """state_dict names of every sparse conv weight under `model`: the tensors whose layout differs between spconv 1.x and 2.x"""
    found = set()
    for name, child in model.named_children():
        path = '%s.%s' % (prefix, name) if prefix else name
        if isinstance(child, spconv.SparseConvolution):
            found.add(path + '.weight')
        found |= find_all_spconv_keys(child, prefix=path)
    return found


def replace_feature(out, new_features):
    return out.replace_feature(new_features)
