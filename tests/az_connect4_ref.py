"""Test infrastructure: the Connect4 simulate env of the reference AlphaZero search (zoo/board_games/connect4/envs/
connect4_env.py: board int[42] row-major 6 x 7 with row 0 on top, values 0 / 1 / 2) in plain Python, and
oracle.az_oracle's search loop over it (same Node, ucb, expand, flatten, noise_table)."""
import numpy as np

from oracle.az_oracle import Node, expand, f32, flatten, noise_table, ucb

# every line of four: (row, column) of its first cell and its direction
LINES = [(r, c, dr, dc) for dr, dc in ((0, 1), (1, 0), (1, 1), (-1, 1)) for r in range(6) for c in range(7)
         if 0 <= r + 3 * dr < 6 and c + 3 * dc < 7]


def done_winner(board):
    """get_done_winner: player 1's lines of four, then player 2's; neither and a full board is a draw"""
    b = np.asarray(board).reshape(6, 7)
    for piece in (1, 2):
        for r, c, dr, dc in LINES:
            if all(b[r + k * dr, c + k * dc] == piece for k in range(4)):
                return True, piece
    return (True, -1) if all(x in (1, 2) for x in b.reshape(-1)) else (False, -1)


class SimConnect4:
    def reset(self, start_player_index=0, board=None):
        self.board = np.zeros(42, np.int32) if board is None else np.array(board, np.int32).reshape(42)
        self.current_player = 1 if start_player_index == 0 else 2

    @property
    def legal_actions(self):
        return [a for a in range(7) if self.board[a] == 0]

    def step(self, action):
        for i in range(35 + action, -1, -7):  # the highest-index empty cell of the column
            if self.board[i] == 0:
                self.board[i] = self.current_player
                break
        self.current_player = 3 - self.current_player

    def get_done_winner(self):
        return done_winner(self.board)


def play(moves, start_player_index=0):
    """the board after `moves` from the empty board, and the index of the player to move"""
    env = SimConnect4()
    env.reset(start_player_index)
    for a in moves:
        env.step(a)
    return env.board.copy(), env.current_player - 1


def encode(board, player):
    """current_state()[1] with scale=True: float32 [3, 6, 7]"""
    b = np.asarray(board).reshape(6, 7)
    return np.stack([b == player, b == 3 - player, np.full((6, 7), player)]).astype(np.float32) / 2


def search(board, start_player_index, sims, pv, sample, base=19652.0, init=1.25, alpha=0.3, frac=0.25):
    """oracle.az_oracle.search's loop over SimConnect4. pv(board [42], legal, player to move) -> ({action: prior},
    value). Returns (root visit counts [7], root children's value_sum float32 [7], flatten(..., priors=True))."""
    env = SimConnect4()
    root, order = Node(), []

    def pv_env(bd, legal):
        return pv(bd, legal, env.current_player)
    env.reset(start_player_index, board)
    expand(root, env, pv_env, order)
    if sample:
        acts = sorted(root.children)
        nz = noise_table(alpha)[len(acts) - 1]
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
    visits, vsums = np.zeros(7, np.int64), np.zeros(7, np.float32)
    for a, c in root.children.items():
        visits[a], vsums[a] = c.visit, c.value_sum
    return visits, vsums, flatten(root, order, priors=True)
