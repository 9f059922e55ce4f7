"""Test infrastructure: the Gomoku simulate env of the reference AlphaZero search (zoo/board_games/gomoku/envs/
gomoku_env.py with board_size 6, get_done_winner_cython.pyx: board int[36] row-major 6 x 6, values 0 / 1 / 2) in
plain Python, and oracle.az_oracle's search loop over it (same Node, ucb, expand, flatten, noise_table)."""
import numpy as np

from oracle.az_oracle import Node, expand, f32, flatten, noise_table, ucb

N = 6
DIRECTIONS = ((1, -1), (1, 0), (1, 1), (0, 1))  # (row, column) steps, in the order the scan tries them
# every line of five: (row, column) of its first cell in row-major order and its direction: 32 on a 6 x 6 board
LINES = [(r, c, dr, dc) for r in range(N) for c in range(N) for dr, dc in DIRECTIONS
         if 0 <= r + 4 * dr < N and 0 <= c + 4 * dc < N]


def done_winner(board):
    """get_done_winner: cells in row-major order; at each stone the four directions; the first run of five that
    fits on the board gives its stone's player. No five and no empty cell is a draw."""
    b = np.asarray(board).reshape(N, N)
    for r in range(N):
        for c in range(N):
            if b[r, c] == 0:
                continue
            for dr, dc in DIRECTIONS:
                if 0 <= r + 4 * dr < N and 0 <= c + 4 * dc < N and \
                        all(b[r + k * dr, c + k * dc] == b[r, c] for k in range(5)):
                    return True, int(b[r, c])
    return (not (b == 0).any()), -1


class SimGomoku:
    def reset(self, start_player_index=0, board=None):
        self.board = np.zeros(N * N, np.int32) if board is None else np.array(board, np.int32).reshape(N * N)
        self.current_player = 1 if start_player_index == 0 else 2

    @property
    def legal_actions(self):
        return [a for a in range(N * N) if self.board[a] == 0]

    def step(self, action):
        assert self.board[action] == 0
        self.board[action] = self.current_player
        self.current_player = 3 - self.current_player

    def get_done_winner(self):
        return done_winner(self.board)


def encode(board, player):
    """current_state()[1] with scale=True: the stones of the player to move, the stones of `to_play` (the other
    player), the player to move; float32 [3, 6, 6]"""
    b = np.asarray(board).reshape(N, N)
    return np.stack([b == player, b == 3 - player, np.full((N, N), player)]).astype(np.float32) / 2


def search(board, start_player_index, sims, pv, sample, base=19652.0, init=1.25, alpha=0.3, frac=0.25):
    """oracle.az_oracle.search's loop over SimGomoku. pv(board [36], legal, player to move) -> ({action: prior},
    value). Returns (root visit counts [36], root children's value_sum float32 [36], flatten(..., priors=True))."""
    env = SimGomoku()
    root, order = Node(), []

    def pv_env(bd, legal):
        return pv(bd, legal, env.current_player)
    env.reset(start_player_index, board)
    expand(root, env, pv_env, order)
    if sample:
        acts = sorted(root.children)
        nz = noise_table(alpha, N * N)[len(acts) - 1]
        for i, a in enumerate(acts):
            c = root.children[a]
            c.prior = f32(float(c.prior) * (1 - frac) + nz[i] * frac)
    for _ in range(sims):
        env.reset(start_player_index, board)
        node = root
        while node.children:
            best, action, child = -9999999.0, -1, None
            legal = set(env.legal_actions)
            for a in sorted(node.children):
                if a in legal:
                    s = ucb(node, node.children[a], base, init)
                    if s > best:
                        best, action, child = s, a, node.children[a]
            if child is None:
                break
            env.step(action)
            node = child
        done, winner = env.get_done_winner()
        if not done:
            leaf = expand(node, env, pv_env, order)
        else:
            leaf = 0.0 if winner == -1 else (1.0 if env.current_player == winner else -1.0)
        node.update_recursive(-leaf)
    visits, vsums = np.zeros(N * N, np.int64), np.zeros(N * N, np.float32)
    for a, c in root.children.items():
        visits[a], vsums[a] = c.visit, c.value_sum
    return visits, vsums, flatten(root, order, priors=True)
