"""Drop-in for ``lzero.mcts.ctree.ctree_stochastic_muzero.stochastic_mz_tree`` (stochastic_mz_tree.pyx:6-90),
GPU-backed."""
from ._tree_api import (MinMaxStatsList, ResultsWrapper, _stochastic_backprop, _stochastic_traverse,
                        _StochasticRootsBase)

__all__ = ["MinMaxStatsList", "ResultsWrapper", "Roots", "batch_traverse", "batch_backpropagate"]


class Roots(_StochasticRootsBase):
    """stochastic_mz_tree.pyx:27-59: Roots(root_num, legal_actions_list, chance_space_size) with prepare,
    prepare_no_noise, get_trajectories (actions and outcomes alternate), get_distributions, get_values, clear, num."""


def batch_traverse(roots, pb_c_base, pb_c_init, discount_factor, min_max_stats_lst, results, virtual_to_play_batch,
                   seed=None):
    """stochastic_mz_tree.pyx:85-90 -> (leaf_node_is_chance, latent_state_index_in_search_path,
    latent_state_index_in_batch, last_actions, virtual_to_play_batchs). seed (not in the reference): this walk's
    Philox key instead of the host seed source; tie and chance draws are per-root streams (include/lzmcts.h)."""
    return _stochastic_traverse(roots, pb_c_base, pb_c_init, discount_factor, min_max_stats_lst, results,
                                virtual_to_play_batch, seed)


def batch_backpropagate(current_latent_state_index, discount_factor, value_prefixs, values, policies,
                        min_max_stats_lst, results, to_play_batch, is_chance_list, leaf_idx_list):
    """stochastic_mz_tree.pyx:75-83."""
    _stochastic_backprop(current_latent_state_index, discount_factor, value_prefixs, values, policies,
                         min_max_stats_lst, results, to_play_batch, is_chance_list, leaf_idx_list)
