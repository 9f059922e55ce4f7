"""Drop-in for ``lzero.mcts.ctree.ctree_sampled_efficientzero.ezs_tree`` (ezs_tree.pyx:6-121), GPU-backed."""
from ._tree_api import MinMaxStatsList, ResultsWrapper, _sampled_backprop, _sampled_traverse, _SampledRootsBase

__all__ = ["MinMaxStatsList", "ResultsWrapper", "Roots", "batch_traverse", "batch_backpropagate"]


class Roots(_SampledRootsBase):
    """ezs_tree.pyx:37-86: Roots(root_num, legal_actions_list, action_space_size, num_of_sampled_actions,
    continuous_action_space) with prepare, prepare_no_noise, get_trajectories (slot indices), get_distributions,
    get_sampled_actions, get_values, clear, num."""


def batch_traverse(roots, pb_c_base, pb_c_init, discount_factor, min_max_stats_lst, results, virtual_to_play_batch,
                   continuous_action_space, seed=None):
    """ezs_tree.pyx:115-121 -> (latent_state_index_in_search_path, latent_state_index_in_batch, last_actions,
    virtual_to_play_batchs). seed (not in the reference): the Philox key of this walk's tie draws and of the
    actions the following batch_backpropagate samples, instead of the host seed source."""
    return _sampled_traverse(roots, pb_c_base, pb_c_init, discount_factor, min_max_stats_lst, results,
                             virtual_to_play_batch, continuous_action_space, seed)


def batch_backpropagate(current_latent_state_index, discount_factor, value_prefixs, values, policies, min_max_stats_lst,
                        results, is_reset_list, to_play_batch):
    """ezs_tree.pyx:103-113."""
    _sampled_backprop(current_latent_state_index, discount_factor, value_prefixs, values, policies, min_max_stats_lst,
                      results, is_reset_list, to_play_batch)
