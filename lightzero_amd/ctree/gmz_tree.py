"""Drop-in for ``lzero.mcts.ctree.ctree_gumbel_muzero.gmz_tree`` (gmz_tree.pyx:5-95), GPU-backed."""
from ._tree_api import MinMaxStatsList, ResultsWrapper, _gumbel_backprop, _gumbel_traverse, _GumbelRootsBase

__all__ = ["MinMaxStatsList", "ResultsWrapper", "Roots", "batch_traverse", "batch_back_propagate"]


class Roots(_GumbelRootsBase):
    """gmz_tree.pyx:28-65: prepare, prepare_no_noise, get_trajectories, get_distributions, get_children_values,
    get_policies, get_values, clear, num."""


def batch_traverse(roots, num_simulations, max_num_considered_actions, discount, results, virtual_to_play_batch):
    """gmz_tree.pyx:91-95 -> (latent_state_index_in_search_path, latent_state_index_in_batch, last_actions,
    virtual_to_play_batchs). No random draw: root selection is sequential halving over the roots' fixed Gumbel
    vector, interior selection an argmax over completed Q values."""
    return _gumbel_traverse(roots, num_simulations, max_num_considered_actions, discount, results,
                            virtual_to_play_batch)


def batch_back_propagate(current_latent_state_index, discount, value_prefixs, values, policies, min_max_stats_lst,
                         results, to_play_batch):
    """gmz_tree.pyx:81-88."""
    _gumbel_backprop(current_latent_state_index, discount, value_prefixs, values, policies, min_max_stats_lst,
                     results, to_play_batch)
