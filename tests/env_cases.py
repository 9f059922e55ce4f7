"""Constructed states of the two stand-in games at the edges play never reaches (helper module, no tests).

Each case is one env step from a written state: (name, state dict as the restatement's new_state, action,
property). The property is a dict of what the step must give — fields of the new state, `pts` (the raw points),
`term` (terminated) — worked out by hand from the specification comments at the top of csrc/lzm_atari.h, not by
running the restatement; a value may be a function of the serve draw. tests/test_env_cases.py runs
oracle/breakout_synth.step / oracle/pong_synth.step on every case for each value of the serve draw and asserts the
property, so no case silently tests something else; tests/test_gpu_env_edges.py puts case i into env i of one
launch of the collect kernels and compares the device with the restatement word for word.

A case also carries the collect step's episode bookkeeping: `score` (the AT_SCORE / PG_SCORE word before the
step), `steps` (steps taken in the episode; MAX_STEPS is the launch's max_episode_steps) and `ep_count`.

The converters map the restatement's dicts to the 16 device words (the order of AT_* / PG_* in lzm_atari.h) and
back. Breakout's 90 brick bits go into three signed int32 words: full words 0 and 1 are -1.
"""
from collections import namedtuple

from oracle import breakout_synth as bk
from oracle import pong_synth as pg

MAX_STEPS = 6  # the launches' max_episode_steps (the truncation cases sit at MAX_STEPS - 1 and - 2)
STATE_WORDS = 16
FULL = bk.FULL_BRICKS

Case = namedtuple("Case", "name state action prop score steps ep_count")

AT_WORDS = ("paddle", "bx", "by", "vx", "vy", "in_play", "brick0", "brick1", "brick2", "lives", "idle", "score")
PG_WORDS = ("paddle", "bx", "by", "vx", "vy", "in_play", "opp", "me", "them", "unused", "idle", "score")
NOOP, FIRE, RIGHT, LEFT, RIGHTFIRE, LEFTFIRE = range(6)


def _s32(w):
    w &= 0xffffffff
    return w - (1 << 32) if w >= (1 << 31) else w


def breakout_words(s, score=0):
    """the restatement's dict -> the 16 int32 device words"""
    b = s["bricks"]
    w = [s["paddle"], s["bx"], s["by"], s["vx"], s["vy"], s["in_play"], _s32(b), _s32(b >> 32), _s32(b >> 64),
         s["lives"], s["idle"], int(score)]
    return w + [0] * (STATE_WORDS - len(w))


def breakout_state(w):
    """the 16 device words -> (the restatement's dict, score)"""
    w = [int(x) for x in w]
    bricks = (w[6] & 0xffffffff) | ((w[7] & 0xffffffff) << 32) | ((w[8] & 0xffffffff) << 64)
    return dict(paddle=w[0], bx=w[1], by=w[2], vx=w[3], vy=w[4], in_play=w[5], bricks=bricks, lives=w[9],
                idle=w[10]), w[11]


def pong_words(s, score=0):
    w = [s["paddle"], s["bx"], s["by"], s["vx"], s["vy"], s["in_play"], s["opp"], s["me"], s["them"], 0, s["idle"],
         int(score)]
    return w + [0] * (STATE_WORDS - len(w))


def pong_state(w):
    w = [int(x) for x in w]
    return dict(paddle=w[0], opp=w[6], bx=w[1], by=w[2], vx=w[3], vy=w[4], in_play=w[5], me=w[7], them=w[8],
                idle=w[10]), w[11]


def words(game, s, score=0):
    return breakout_words(s, score) if game == "breakout" else pong_words(s, score)


def state_of(game, w):
    return breakout_state(w) if game == "breakout" else pong_state(w)


def synth(game):
    return bk if game == "breakout" else pg


def draws(game):
    """every value of the serve draw, as the restatement's step takes it"""
    return (1, -1) if game == "breakout" else (0, 1, 2, 3)


def draw_from_bits(game, b0, b1):
    """the restatement's serve argument from collect_rng.serve_bits' two bits of one env"""
    return (1 if b0 else -1) if game == "breakout" else (int(b0) | (int(b1) << 1))


def serves(game, s, action):
    """whether this step draws the serve (the ball is not in play, and FIRE or the idle count serves it)"""
    fire = action == FIRE if game == "breakout" else action in (FIRE, RIGHTFIRE, LEFTFIRE)
    return (not s["in_play"]) and (fire or s["idle"] + 1 >= bk.AUTO_SERVE)


# ------------------------------------------------------------------------------------------------ Breakout
def brick(r, c):
    return 1 << (r * bk.BRICK_COLS + c)


def rows_upto(r):
    """rows 0 .. r full, the rows below them empty"""
    return (1 << ((r + 1) * bk.BRICK_COLS)) - 1


def _bk(paddle=27, bx=0, by=0, vx=0, vy=0, in_play=1, bricks=FULL, lives=1, idle=0):
    return dict(paddle=paddle, bx=bx, by=by, vx=vx, vy=vy, in_play=in_play, bricks=bricks, lives=lives, idle=idle)


def _idle(paddle, idle=0):
    return _bk(paddle=paddle, in_play=0, idle=idle)


def _breakout_cases():
    out = []

    def add(name, state, action, score=0, steps=0, ep_count=0, **prop):
        prop.setdefault("pts", 0.0)
        prop.setdefault("term", False)
        out.append(Case(name, state, action, prop, score, steps, ep_count))

    # ---- paddle: 3 columns per step, clamped to [2, 54]
    for p in (2, 3, 4, 5):
        add(f"left_from_{p}", _idle(p), LEFT, paddle=2, idle=1, in_play=0)
    for p in (51, 52, 53, 54):
        add(f"right_from_{p}", _idle(p), RIGHT, paddle=54, idle=1, in_play=0)
    add("left_from_30", _idle(30), LEFT, paddle=27, idle=1)
    add("right_from_30", _idle(30), RIGHT, paddle=33, idle=1)
    add("noop_leaves_paddle", _idle(30), NOOP, paddle=30, idle=1, in_play=0)
    add("fire_leaves_paddle", _idle(30), FIRE, paddle=30, in_play=1)
    # the ball in free flight: 2 sub-steps of (1, -1) from (30, 30)
    add("fire_in_play_does_nothing", _bk(bx=30, by=30, vx=1, vy=-1), FIRE, paddle=27, bx=32, by=28, vx=1, vy=-1,
        in_play=1, idle=0, bricks=FULL)
    add("noop_in_play", _bk(bx=30, by=30, vx=1, vy=-1), NOOP, paddle=27, bx=32, by=28, vx=1, vy=-1, in_play=1, idle=0)
    # ---- serve
    add("idle_6_noop_no_serve", _idle(30, 6), NOOP, idle=7, in_play=0, bx=0, by=0, vx=0, vy=0)
    add("idle_7_noop_auto_serve", _idle(30, 7), NOOP, idle=0, in_play=1, bx=33, by=50, vx=lambda d: d, vy=-1)
    add("fire_at_idle_0", _idle(30, 0), FIRE, idle=0, in_play=1, bx=33, by=50, vx=lambda d: d, vy=-1, paddle=30)
    add("fire_at_idle_5", _idle(12, 5), FIRE, idle=0, in_play=1, bx=15, by=50, vx=lambda d: d, vy=-1)
    add("serve_after_move_right", _idle(40, 7), RIGHT, paddle=43, in_play=1, bx=46, by=50, vx=lambda d: d, vy=-1)
    add("serve_after_clamped_left", _idle(3, 7), LEFT, paddle=2, in_play=1, bx=5, by=50, vx=lambda d: d, vy=-1)
    add("serve_after_clamped_right", _idle(53, 7), RIGHT, paddle=54, in_play=1, bx=57, by=50, vx=lambda d: d, vy=-1)
    for k in range(6):  # more serves, so that a launch sees both directions
        add(f"fire_serve_{k}", _idle(10 + 7 * k), FIRE, in_play=1, bx=13 + 7 * k, by=50, vx=lambda d: d, vy=-1)
    # ---- side walls (the ball's column stays in [2, 60]); y 35 -> 37 is free flight
    for x, vx, ex, evx, sub in ((2, -1, 3, 1, 1), (3, -1, 2, 1, 2), (2, -2, 4, 2, 1), (3, -2, 4, 2, 1), (4, -2, 2, 2, 2),
                                (5, -2, 2, 2, 2), (4, -1, 2, -1, 0),
                                (60, 1, 59, -1, 1), (59, 1, 60, -1, 2), (60, 2, 58, -2, 1), (59, 2, 58, -2, 1),
                                (58, 2, 60, -2, 2), (57, 2, 60, -2, 2), (58, 1, 60, 1, 0)):
        add(f"side_wall_x{x}_vx{vx}_sub{sub}", _bk(bx=x, by=35, vx=vx, vy=1), NOOP, bx=ex, vx=evx, by=37, vy=1)
    # ---- top wall (rows 0, 1): the gap above the bricks is free
    add("top_wall_y2_sub1", _bk(bx=30, by=2, vx=1, vy=-1), NOOP, bx=32, by=3, vy=1, vx=1)
    add("top_wall_y3_sub2", _bk(bx=30, by=3, vx=1, vy=-1), NOOP, bx=32, by=2, vy=1, vx=1)
    add("top_wall_y4_none", _bk(bx=30, by=4, vx=1, vy=-1), NOOP, bx=32, by=2, vy=-1, vx=1)
    add("corner_top_left", _bk(bx=2, by=2, vx=-1, vy=-1), NOOP, bx=3, by=3, vx=1, vy=1)
    add("corner_top_right", _bk(bx=60, by=2, vx=1, vy=-1), NOOP, bx=59, by=3, vx=-1, vy=1)
    add("corner_top_left_vx2", _bk(bx=3, by=2, vx=-2, vy=-1), NOOP, bx=4, by=3, vx=2, vy=1)
    # ---- bricks. Row r covers y in [8 + 2r, 10 + 2r), column c x in [2 + 4c, 6 + 4c).
    # from below, only row r standing: sub-step 1 puts the ball's top-left pixel at (11, 9 + 2r): brick (r, 2); the
    # ball turns back at its old y and sub-step 2 is free flight
    for r, pts in enumerate((7, 7, 4, 4, 1, 1)):
        row = rows_upto(r) & ~(rows_upto(r - 1) if r else 0)
        add(f"row{r}_from_below", _bk(bx=10, by=10 + 2 * r, vx=1, vy=-1, bricks=row), NOOP, score=3, pts=float(pts),
            bricks=row & ~brick(r, 2), bx=12, by=11 + 2 * r, vx=1, vy=1)
    # from above, out of the gap under the top wall: the ball's lower pixels (k = 2) reach row 0
    add("row0_from_above", _bk(bx=10, by=6, vx=1, vy=1), NOOP, pts=7.0, bricks=FULL & ~brick(0, 2), bx=12, by=5, vx=1,
        vy=-1)
    # the first and last bit of each word (rows above the brick full, rows below empty: nothing else is hit)
    for b in (0, 31, 32, 63, 64, 89):
        r, c = divmod(b, bk.BRICK_COLS)
        pts = (7, 7, 4, 4, 1, 1)[r]
        add(f"brick_index_{b}", _bk(bx=3 + 4 * c, by=10 + 2 * r, vx=-1, vy=-1, bricks=rows_upto(r)), NOOP,
            pts=float(pts), bricks=rows_upto(r) & ~(1 << b), bx=max(1 + 4 * c, 2), by=11 + 2 * r, vx=-1 if c else 1, vy=1)
        # (column 0: sub-step 2 meets the left wall)
    # two live bricks under the ball: the first in pixel order (0,0), (1,0), (0,1), (1,1) breaks
    add("two_bricks_side_by_side", _bk(bx=28, by=16, vx=1, vy=-1, bricks=brick(3, 6) | brick(3, 7)), NOOP, pts=4.0,
        bricks=brick(3, 7), bx=30, by=17, vx=1, vy=1)
    # stacked, met in sub-step 2 (sub-step 1 lies over the hole of column 4)
    add("two_bricks_stacked", _bk(bx=18, by=15, vx=2, vy=-1, bricks=brick(2, 5) | brick(3, 5)), NOOP, pts=4.0,
        bricks=brick(3, 5), bx=22, by=14, vx=2, vy=1)
    # pixel (0,0) over a hole, (1,0) over a brick: that one breaks
    add("second_pixel_hits", _bk(bx=28, by=16, vx=1, vy=-1, bricks=brick(3, 7) | brick(0, 0)), NOOP, pts=4.0,
        bricks=brick(0, 0), bx=30, by=17, vx=1, vy=1)
    # pixels (0,0), (1,0) over holes, (0,1) over a hole, (1,1) over a brick, moving down
    add("fourth_pixel_hits", _bk(bx=28, by=12, vx=1, vy=1, bricks=brick(3, 7) | brick(0, 0)), NOOP, pts=4.0,
        bricks=brick(0, 0), bx=30, by=11, vx=1, vy=-1)
    add("hole_passes", _bk(bx=10, by=20, vx=1, vy=-1, bricks=FULL & ~brick(5, 2)), NOOP, bricks=FULL & ~brick(5, 2),
        bx=12, by=18, vx=1, vy=-1)
    # a hit in both sub-steps against the full wall: row r from below, then row r + 1 on the way back
    for r, pts in ((0, 14), (1, 11), (2, 8), (3, 5), (4, 2)):
        add(f"double_hit_{pts}", _bk(bx=10, by=10 + 2 * r, vx=1, vy=-1), NOOP, score=100, pts=float(pts),
            bricks=FULL & ~brick(r, 2) & ~brick(r + 1, 2), bx=12, by=10 + 2 * r, vx=1, vy=-1)
    add("hit_and_side_wall", _bk(bx=2, by=20, vx=-1, vy=-1), NOOP, pts=1.0, bricks=FULL & ~brick(5, 0), bx=3, by=21,
        vx=1, vy=1)
    add("hit_and_right_wall", _bk(bx=60, by=20, vx=1, vy=-1), NOOP, pts=1.0, bricks=FULL & ~brick(5, 14), bx=59, by=21,
        vx=-1, vy=1)
    add("hit_keeps_old_y", _bk(bx=20, by=21, vx=1, vy=-1), NOOP, pts=1.0, bricks=FULL & ~brick(5, 5), bx=22, by=20,
        vx=1, vy=1)  # sub-step 1 free to y 20, sub-step 2 hits at y 19 and stays at 20
    # ---- the wall cleared
    add("last_brick_word2", _bk(bx=10, by=20, vx=1, vy=-1, bricks=brick(5, 2)), NOOP, score=431, pts=1.0, bricks=FULL,
        bx=12, by=21, vx=1, vy=1)
    add("last_brick_word1", _bk(bx=10, by=14, vx=1, vy=-1, bricks=brick(2, 12)), NOOP, pts=0.0, bricks=brick(2, 12),
        bx=12, by=12, vx=1, vy=-1)  # (column 12 is elsewhere: a pass over holes, no refill)
    add("last_brick_word1_hit", _bk(bx=49, by=14, vx=1, vy=-1, bricks=brick(2, 12)), NOOP, pts=4.0, bricks=FULL, bx=51,
        by=15, vx=1, vy=1)
    add("last_brick_word0", _bk(bx=21, by=10, vx=1, vy=-1, bricks=brick(0, 5)), NOOP, pts=7.0, bricks=FULL, bx=23,
        by=11, vx=1, vy=1)
    add("two_left_one_hit", _bk(bx=10, by=20, vx=1, vy=-1, bricks=brick(5, 2) | brick(0, 0)), NOOP, pts=1.0,
        bricks=brick(0, 0), bx=12, by=21, vx=1, vy=1)
    add("two_left_one_hit_word1", _bk(bx=10, by=20, vx=1, vy=-1, bricks=brick(5, 2) | brick(3, 3)), NOOP, pts=1.0,
        bricks=brick(3, 3))
    add("two_left_one_hit_word2", _bk(bx=21, by=10, vx=1, vy=-1, bricks=brick(0, 5) | brick(5, 14)), NOOP, pts=7.0,
        bricks=brick(5, 14))
    # ---- the paddle (row 58, columns px .. px + 7) turns a falling ball back; off = (nx + 1) - (px + 4)
    for off in range(-4, 5):
        nvx = -2 if off < -2 else (-1 if off < 0 else (1 if off < 2 else 2))
        nx = 33 + off
        add(f"paddle_off_{off}", _bk(paddle=30, bx=nx - 1, by=56, vx=1, vy=1), NOOP, bx=nx + nvx, by=55, vx=nvx, vy=-1,
            in_play=1)
    add("paddle_miss_left", _bk(paddle=30, bx=29, by=56, vx=-1, vy=1), NOOP, bx=27, by=58, vx=-1, vy=1)
    add("paddle_miss_right", _bk(paddle=30, bx=37, by=56, vx=1, vy=1), NOOP, bx=39, by=58, vx=1, vy=1)
    add("paddle_second_substep", _bk(paddle=30, bx=31, by=55, vx=1, vy=1), NOOP, bx=33, by=56, vx=1, vy=-1)
    add("paddle_ny_59", _bk(paddle=30, bx=32, by=58, vx=1, vy=1), NOOP, bx=34, by=55, vx=1, vy=-1)
    add("paddle_ny_60_past", _bk(paddle=30, bx=32, by=59, vx=1, vy=1), NOOP, bx=34, by=61, vx=1, vy=1, in_play=1)
    add("ball_up_beside_paddle", _bk(paddle=30, bx=32, by=59, vx=1, vy=-1), NOOP, bx=34, by=57, vx=1, vy=-1)
    add("paddle_moves_into_path", _bk(paddle=27, bx=35, by=56, vx=1, vy=1), RIGHT, paddle=30, bx=38, by=55, vx=2, vy=-1)
    add("paddle_moves_out_of_path", _bk(paddle=30, bx=35, by=56, vx=1, vy=1), LEFT, paddle=27, bx=37, by=58, vx=1, vy=1)
    # ---- the ball lost (y > 62): one life per episode
    add("lost_sub1", _bk(bx=20, by=62, vx=1, vy=1), NOOP, score=9, term=True, in_play=0, lives=0, bx=21, by=63, vx=1,
        vy=1)
    add("lost_sub2", _bk(bx=20, by=61, vx=-2, vy=1), NOOP, score=66, term=True, in_play=0, lives=0, bx=16, by=63)
    add("lost_with_two_lives", _bk(bx=20, by=62, vx=1, vy=1, lives=2), NOOP, term=False, in_play=0, lives=1, by=63)
    add("y_62_not_lost", _bk(bx=20, by=60, vx=1, vy=1), NOOP, in_play=1, lives=1, by=62, bx=22)
    # ---- truncation at max_episode_steps
    add("truncated", _idle(30), NOOP, steps=MAX_STEPS - 1, score=12, done=True, term=False)
    add("truncated_and_lost", _bk(bx=20, by=62, vx=1, vy=1), NOOP, steps=MAX_STEPS - 1, score=5, done=True, term=True)
    add("truncated_with_points", _bk(bx=10, by=10, vx=1, vy=-1), NOOP, steps=MAX_STEPS - 1, score=50, done=True,
        pts=14.0)
    add("one_before_truncation", _idle(30), NOOP, steps=MAX_STEPS - 2, done=False)
    add("lost_mid_episode_second_slot", _bk(bx=20, by=62, vx=1, vy=1), NOOP, steps=3, ep_count=1, score=21, done=True,
        term=True)
    return out


# ------------------------------------------------------------------------------------------------ Pong
def _pg(paddle=28, opp=27, bx=30, by=30, vx=1, vy=1, in_play=1, me=0, them=0, idle=0):
    return dict(paddle=paddle, opp=opp, bx=bx, by=by, vx=vx, vy=vy, in_play=in_play, me=me, them=them, idle=idle)


def _bounce(off):
    return -2 if off < -2 else (-1 if off < 0 else (1 if off < 2 else 2))


def _pong_cases():
    out = []

    def add(name, state, action, score=0, steps=0, ep_count=0, **prop):
        prop.setdefault("pts", 0.0)
        prop.setdefault("term", False)
        out.append(Case(name, state, action, prop, score, steps, ep_count))

    svx, svy = (lambda d: 1 if d & 1 else -1), (lambda d: 1 if d & 2 else -1)
    # ---- the six actions at the clamps (rows [2, 54]); RIGHT is up (-3), LEFT down (+3); the FIRE ones serve
    for p in (2, 3, 4, 52, 53, 54):
        for a in range(6):
            up, down, fire = a in (RIGHT, RIGHTFIRE), a in (LEFT, LEFTFIRE), a in (FIRE, RIGHTFIRE, LEFTFIRE)
            want = max(p - 3, 2) if up else (min(p + 3, 54) if down else p)
            if fire:
                add(f"action_{a}_from_{p}", _pg(paddle=p, in_play=0, bx=0, by=0, vx=0, vy=0), a, paddle=want, in_play=1,
                    idle=0, bx=31, by=31, vx=svx, vy=svy, opp=27)
            else:
                add(f"action_{a}_from_{p}", _pg(paddle=p, in_play=0, bx=0, by=0, vx=0, vy=0), a, paddle=want, in_play=0,
                    idle=1, bx=0, by=0, vx=0, vy=0, opp=27)
    add("idle_6_noop_no_serve", _pg(in_play=0, idle=6, bx=0, by=0, vx=0, vy=0), NOOP, in_play=0, idle=7)
    add("idle_7_noop_auto_serve", _pg(in_play=0, idle=7, bx=0, by=0, vx=0, vy=0), NOOP, in_play=1, idle=0, bx=31, by=31,
        vx=svx, vy=svy)
    add("idle_7_up_auto_serve", _pg(paddle=30, in_play=0, idle=7, bx=0, by=0, vx=0, vy=0), RIGHT, paddle=27, in_play=1,
        idle=0, bx=31, by=31, vx=svx, vy=svy)
    add("fire_in_play_does_nothing", _pg(), FIRE, bx=32, by=32, vx=1, vy=1, opp=27, idle=0, paddle=28)
    # ---- top and bottom walls (the ball's row stays in [2, 60]); the opponent is held at its clamp
    for y, vy, ey, evy, sub in ((2, -1, 3, 1, 1), (3, -1, 2, 1, 2), (3, -2, 4, 2, 1), (4, -2, 2, 2, 2), (4, -1, 2, -1, 0)):
        add(f"top_wall_y{y}_vy{vy}_sub{sub}", _pg(opp=2, by=y, vy=vy), NOOP, by=ey, vy=evy, bx=32, vx=1, opp=2)
    for y, vy, ey, evy, sub in ((60, 1, 59, -1, 1), (59, 1, 60, -1, 2), (59, 2, 58, -2, 1), (58, 2, 60, -2, 2),
                                (58, 1, 60, 1, 0)):
        add(f"bottom_wall_y{y}_vy{vy}_sub{sub}", _pg(opp=54, by=y, vy=vy), NOOP, by=ey, vy=evy, bx=32, vx=1, opp=54)
    # ---- the agent's paddle (columns 56, 57, rows py .. py + 7): off = (ny + 1) - (py + 4). The opponent, at its
    # top clamp and far above the ball, comes down 2 rows per sub-step.
    for off in range(-4, 5):
        ny, nvy = 33 + off, _bounce(off)
        add(f"agent_off_{off}", _pg(paddle=30, opp=2, bx=54, by=ny - 1, vx=1, vy=1), NOOP, bx=53, by=ny + nvy, vx=-1,
            vy=nvy, opp=6)
    add("agent_x_edge_57", _pg(paddle=30, opp=2, bx=56, by=32, vx=1, vy=1), NOOP, bx=53, by=34, vx=-1, vy=1, opp=6)
    add("agent_x_past_58", _pg(paddle=30, opp=2, bx=57, by=32, vx=1, vy=1), NOOP, bx=59, by=34, vx=1, vy=1, opp=6)
    add("agent_second_substep", _pg(paddle=30, opp=2, bx=53, by=31, vx=1, vy=1), NOOP, bx=54, by=33, vx=-1, vy=1, opp=6)
    add("agent_miss_above", _pg(paddle=30, opp=2, bx=54, by=29, vx=1, vy=-1), NOOP, bx=56, by=27, vx=1, vy=-1, opp=6)
    add("agent_miss_below", _pg(paddle=30, opp=2, bx=54, by=37, vx=1, vy=1), NOOP, bx=56, by=39, vx=1, vy=1, opp=6)
    add("agent_ball_moving_away", _pg(paddle=30, opp=2, bx=57, by=32, vx=-1, vy=1), NOOP, bx=55, by=34, vx=-1, vy=1)
    add("agent_moves_into_path", _pg(paddle=33, opp=2, bx=54, by=28, vx=1, vy=1), RIGHT, paddle=30, bx=53, by=27, vx=-1,
        vy=-2)  # off -4 after the move up; a miss before it
    # ---- the opponent's paddle (columns 6, 7, rows oy .. oy + 7), which first tracks the ball in each sub-step.
    # In its dead band (the ball's centre within 1 of its own) it stands still: off - vy_in in [-1, 1].
    for off, vy_in in ((-3, -2), (-2, -1), (-1, -1), (0, 1), (1, 1), (2, 1), (3, 2)):
        ny, nvy = 33 + off, _bounce(off)
        add(f"opp_off_{off}", _pg(opp=30, bx=8, by=ny - vy_in, vx=-1, vy=vy_in), NOOP, bx=9, by=ny + nvy, vx=1, vy=nvy,
            opp=30 + (2 if off > 1 else (-2 if off < -1 else 0)))
    # the contact edges need a move: the opponent steps up from 32 to 30 (down from 28 to 30) and meets the ball
    add("opp_top_edge", _pg(opp=32, bx=8, by=28, vx=-1, vy=1), NOOP, bx=9, by=27, vx=1, vy=-2, opp=28)
    add("opp_bottom_edge", _pg(opp=28, bx=8, by=36, vx=-1, vy=1), NOOP, bx=9, by=39, vx=1, vy=2, opp=32)
    # misses by one row, at the column where the ball leaves the paddle's reach in sub-step 2
    add("opp_miss_above", _pg(opp=32, bx=6, by=27, vx=-1, vy=1), NOOP, bx=4, by=29, vx=-1, vy=1, opp=28)
    add("opp_miss_below", _pg(opp=28, bx=6, by=37, vx=-1, vy=1), NOOP, bx=4, by=39, vx=-1, vy=1, opp=32)
    add("opp_x_edge_5", _pg(opp=30, bx=6, by=32, vx=-1, vy=1), NOOP, bx=9, by=34, vx=1, vy=1, opp=30)
    add("opp_x_past_4", _pg(opp=30, bx=5, by=32, vx=-1, vy=1), NOOP, bx=3, by=34, vx=-1, vy=1, opp=30)
    add("opp_second_substep", _pg(opp=30, bx=9, by=32, vx=-1, vy=1), NOOP, bx=8, by=34, vx=1, vy=1, opp=30)
    add("opp_ball_moving_away", _pg(opp=30, bx=5, by=32, vx=1, vy=1), NOOP, bx=7, by=34, vx=1, vy=1, opp=30)
    # ---- opponent tracking: centre oc = oy + 4 against the ball's bc = y + 1, 2 rows per sub-step
    add("track_band_low", _pg(opp=27, by=29, vy=1), NOOP, opp=27, by=31)
    add("track_band_mid", _pg(opp=27, by=30, vy=1), NOOP, opp=27, by=32)
    add("track_band_high", _pg(opp=27, by=31, vy=-1), NOOP, opp=27, by=29)
    add("track_down_once", _pg(opp=27, by=32, vy=1), NOOP, opp=29, by=34)
    add("track_up_once", _pg(opp=27, by=28, vy=-1), NOOP, opp=25, by=26)
    add("track_down_4_per_step", _pg(opp=27, by=40, vy=1), NOOP, opp=31, by=42)
    add("track_up_4_per_step", _pg(opp=27, by=20, vy=-1), NOOP, opp=23, by=18)
    add("track_clamp_bottom", _pg(opp=53, by=59, vy=1), NOOP, opp=54, by=60, vy=-1)
    add("track_clamp_top", _pg(opp=3, by=2, vy=1), NOOP, opp=2, by=4)
    # ---- points: the ball past a paddle's side (x < 0: the agent's; x > 62: the opponent's)
    add("opp_out_of_reach_pass", _pg(opp=2, bx=8, by=50, vx=-1, vy=1), NOOP, bx=6, by=52, vx=-1, vy=1, opp=6, in_play=1)
    add("agent_point_sub1", _pg(opp=2, bx=0, by=50, vx=-1, vy=1, me=3, them=5), NOOP, score=-2, pts=1.0, me=4, them=5,
        in_play=0, bx=-1, by=51, opp=4)
    add("agent_point_sub2", _pg(opp=2, bx=1, by=50, vx=-1, vy=1, me=0, them=0), NOOP, pts=1.0, me=1, them=0, in_play=0,
        bx=-1, by=52, opp=6)
    add("x_0_no_point", _pg(opp=2, bx=2, by=50, vx=-1, vy=1), NOOP, pts=0.0, me=0, them=0, in_play=1, bx=0, by=52)
    add("opp_point_sub1", _pg(paddle=2, bx=62, by=50, vx=1, vy=1, me=3, them=5), NOOP, score=-2, pts=-1.0, me=3, them=6,
        in_play=0, bx=63, by=51)
    add("opp_point_sub2", _pg(paddle=2, bx=61, by=50, vx=1, vy=1), NOOP, pts=-1.0, me=0, them=1, in_play=0, bx=63, by=52)
    add("x_62_no_point", _pg(paddle=2, bx=60, by=50, vx=1, vy=1), NOOP, pts=0.0, them=0, in_play=1, bx=62, by=52)
    # ---- scores: 21 points for either side end the episode; ep_return is the point difference
    add("agent_20_to_21", _pg(opp=2, bx=0, by=50, vx=-1, vy=1, me=20, them=3), NOOP, score=17, pts=1.0, me=21, them=3,
        term=True)
    add("opp_20_to_21", _pg(paddle=2, bx=62, by=50, vx=1, vy=1, me=5, them=20), NOOP, score=-15, pts=-1.0, me=5, them=21,
        term=True)
    add("both_20_agent_scores", _pg(opp=2, bx=0, by=50, vx=-1, vy=1, me=20, them=20), NOOP, score=0, pts=1.0, me=21,
        them=20, term=True)
    add("both_20_opp_scores", _pg(paddle=2, bx=61, by=50, vx=1, vy=1, me=20, them=20), NOOP, score=0, pts=-1.0, me=20,
        them=21, term=True)
    add("agent_19_to_20", _pg(opp=2, bx=0, by=50, vx=-1, vy=1, me=19, them=20), NOOP, score=-1, pts=1.0, me=20, them=20,
        term=False)
    add("opp_19_to_20", _pg(paddle=2, bx=62, by=50, vx=1, vy=1, me=0, them=19), NOOP, score=-19, pts=-1.0, them=20,
        term=False)
    # ---- truncation
    add("truncated", _pg(), NOOP, steps=MAX_STEPS - 1, score=-4, done=True, term=False)
    add("truncated_with_point", _pg(opp=2, bx=0, by=50, vx=-1, vy=1, me=7, them=2), NOOP, steps=MAX_STEPS - 1, score=5,
        done=True, pts=1.0, term=False)
    add("truncated_and_won", _pg(opp=2, bx=0, by=50, vx=-1, vy=1, me=20, them=2), NOOP, steps=MAX_STEPS - 1, score=18,
        done=True, pts=1.0, term=True)
    add("one_before_truncation", _pg(), NOOP, steps=MAX_STEPS - 2, done=False)
    add("won_mid_episode_second_slot", _pg(opp=2, bx=0, by=50, vx=-1, vy=1, me=20, them=9), NOOP, steps=2, ep_count=1,
        score=11, done=True, pts=1.0, term=True)
    return out


CASES = {"breakout": _breakout_cases(), "pong": _pong_cases()}


def done(case, term):
    """the collect step's episode end: terminated, or the step count reaches MAX_STEPS"""
    return bool(term) or case.steps + 1 >= MAX_STEPS


def check_case(game, case, draw):
    """step the restatement from the case's state under serve draw `draw` and assert the case's property;
    returns (s1, pts, term)"""
    s1, pts, term = synth(game).step(case.state, case.action, draw)
    for k, want in case.prop.items():
        want = want(draw) if callable(want) else want
        got = pts if k == "pts" else (term if k == "term" else (done(case, term) if k == "done" else s1[k]))
        assert got == want, f"{game} case {case.name} (draw {draw}): {k} = {got!r}, the case says {want!r}"
    return s1, pts, term


# ------------------------------------------------------------------------------------------------ lockstep runs
def pong_actions(n, steps, seed=11):
    """seeded uniform actions [steps][n] for the Pong lockstep run"""
    import numpy as np
    return np.random.default_rng(seed).integers(0, 6, (steps, n)).astype(np.int32)


class BreakoutTracker:
    """The scripted Breakout policy of the lockstep run: FIRE when the ball is not in play, otherwise move the
    paddle's centre towards the ball's plus an offset that is drawn anew (seeded) whenever the ball's vertical
    direction changes, so the bounces leave in all four directions."""

    def __init__(self, n, seed=7):
        import numpy as np
        self.rng = np.random.default_rng(seed)
        self.off = self.rng.integers(-3, 4, n)
        self.last_vy = [0] * n

    def __call__(self, t, states):
        import numpy as np
        a = np.zeros(len(states), np.int32)
        for i, s in enumerate(states):
            if not s["in_play"]:
                a[i] = FIRE
                continue
            if s["vy"] != self.last_vy[i]:
                self.last_vy[i] = s["vy"]
                self.off[i] = self.rng.integers(-3, 4)
            target, centre = s["bx"] + 1 + int(self.off[i]), s["paddle"] + bk.PADDLE_W // 2
            a[i] = RIGHT if target > centre + 1 else (LEFT if target < centre - 1 else NOOP)
        return a


def run_restated(game, n, steps, policy, seed, max_steps, first_key=1):
    """`steps` env steps of n envs through the restatement, as the collect kernels run them: the envs start from
    the reset entry point's draw, step t uses the Philox key first_key + t for the serve bits and for the reset
    of the envs whose episode ends in it (collect_rng). policy(t, states) gives the actions [n]. Returns the
    actions [steps][n], the 16 state words after every step [steps][n][16], the step counts [steps][n], and
    counts of what the run met."""
    import numpy as np
    from oracle import collect_rng as cr
    reset = cr.breakout_reset if game == "breakout" else cr.pong_reset
    w0 = reset(seed, n)
    states = [state_of(game, w0[i])[0] for i in range(n)]
    score, count = [0] * n, [0] * n
    actions = np.zeros((steps, n), np.int32)
    out_words = np.zeros((steps, n, STATE_WORDS), np.int32)
    out_steps = np.zeros((steps, n), np.int32)
    met = dict(terminated=0, truncated=0, score_ends=0, points=0.0, upper_rows=0, agent_points=0, refills=0)
    for t in range(steps):
        key = first_key + t
        actions[t] = policy(t, states)
        b0, b1 = cr.serve_bits(seed, n, key)
        wr = None
        for i in range(n):
            s1, pts, term = synth(game).step(states[i], int(actions[t, i]), draw_from_bits(game, b0[i], b1[i]))
            score[i] += int(pts)
            count[i] += 1
            met["points"] += abs(pts)
            met["upper_rows"] += int(pts >= 4)
            met["agent_points"] += int(game == "pong" and pts > 0)
            met["refills"] += int(game == "breakout" and pts > 0 and s1["bricks"] == FULL)
            if term or count[i] >= max_steps:
                met["terminated" if term else "truncated"] += 1
                met["score_ends"] += int(game == "pong" and term)
                wr = reset(seed, n, step=key) if wr is None else wr
                states[i], score[i], count[i] = state_of(game, wr[i])[0], 0, 0
            else:
                states[i] = s1
            out_words[t, i] = words(game, states[i], score[i])
            out_steps[t, i] = count[i]
    return dict(actions=actions, words=out_words, steps=out_steps, first_words=w0, **met)
