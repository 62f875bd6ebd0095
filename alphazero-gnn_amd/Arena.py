"""Arena (reference Arena.py:7-292).  Two-player games: two action functions pitted against each
other, each starting half of the games.  Single-player games (FrozenLake): both players solve
the same board and are compared by success first, then by steps."""
import logging

import numpy as np
from tqdm import tqdm

log = logging.getLogger(__name__)


class Arena:
    def __init__(self, player1, player2, game, display=None):
        self.player1 = player1
        self.player2 = player2
        self.game = game
        self.display = display
        self.is_single_player = hasattr(self.game, "is_two_player") and not self.game.is_two_player

    def playGameForSinglePlayer(self, player, board_state=None, verbose=False):
        """One episode of `player` from `board_state` (default: the init board), at most 5 steps
        per cell -> (result, steps): 1 win, -1 loss, 0 when the cap ran out (Arena.py:29-104).
        An invalid action is replaced by np.random.choice over the valid ones; an exception in
        the player ends the episode where it stands."""
        game = self.game
        board = np.copy(board_state) if board_state is not None else game.getInitBoard()
        nx, ny = game.getBoardSize()
        max_steps = nx * ny * 5
        it = 0
        if hasattr(player, "startGame"):
            player.startGame()
        while game.getGameEnded(board, 1) == 0 and it < max_steps:
            it += 1
            if verbose:
                assert self.display
                print(f"Turn {it}, Player 1")
                self.display(board)
            canonical = game.getCanonicalForm(board, 1)
            try:
                action = player(canonical)
                valids = game.getValidMoves(canonical, 1)
                if valids[action] == 0:
                    log.error(f"Action {action} is not valid!")
                    log.debug(f"valids = {valids}")
                    options = np.where(valids == 1)[0]
                    if len(options) == 0:
                        log.error("No valid actions available!")
                        break
                    action = np.random.choice(options)
                board, _ = game.getNextState(board, 1, action)
            except Exception as e:
                log.error(f"Error during gameplay: {e}")
                break
        if hasattr(player, "endGame"):
            player.endGame()
        result = game.getGameEnded(board, 1)
        if verbose:
            assert self.display
            print(f"Game over: Turn {it}, Result {result}")
            self.display(board)
        if it >= max_steps and result == 0:
            return 0, it
        return result, it

    def playGamesForSinglePlayer(self, num, verbose=False):
        """num boards, each played once by either player -> (player1 better, player2 better,
        equal) (Arena.py:166-247): a success beats a failure; of two successes the one with
        fewer steps wins; of two losses the one that survived longer; anything else is a draw."""
        one = two = draws = 0
        steps = [0, 0]
        wins = [0, 0]
        for _ in tqdm(range(num), desc="Arena.playGames (Single-Player)"):
            board = self.game.getInitBoard()
            r1, s1 = self.playGameForSinglePlayer(self.player1, board)
            r2, s2 = self.playGameForSinglePlayer(self.player2, board)
            steps[0] += s1
            steps[1] += s2
            wins[0] += r1 > 0
            wins[1] += r2 > 0
            if (r1 > 0) != (r2 > 0):
                better = 1 if r1 > 0 else 2
            elif r1 > 0:                          # both succeeded: fewer steps
                better = 1 if s1 < s2 else 2 if s2 < s1 else 0
            elif r1 < 0 and r2 < 0:               # both fell in: the longer survivor
                better = 1 if s1 > s2 else 2 if s2 > s1 else 0
            else:
                better = 0
            one += better == 1
            two += better == 2
            draws += better == 0
        log.info(f"Results - Player1 wins: {one}, Player2 wins: {two}, Draws: {draws}")
        if num > 0:
            log.info(f"Success rates - Player1: {wins[0] / num:.2f}, Player2: {wins[1] / num:.2f}")
            for i in (0, 1):
                if wins[i] > 0:
                    log.info(f"Avg steps for success - Player{i + 1}: {steps[i] / wins[i]:.2f}")
        return one, two, draws

    def playGame(self, verbose=False):
        """Player 1's result of one single-player episode, or one two-player game."""
        if self.is_single_player:
            return self.playGameForSinglePlayer(self.player1, verbose=verbose)[0]
        return self.playGameForTwoPlayer(verbose=verbose)

    def playGameForTwoPlayer(self, verbose=False):
        """One game; returns +1 if player1 won, -1 if player2 won, the draw value otherwise
        (curPlayer * getGameEnded(board, curPlayer), Arena.py:152)."""
        players = {1: self.player1, -1: self.player2}
        cur = 1
        board = self.game.getInitBoard()
        it = 0
        for p in (self.player2, self.player1):
            if hasattr(p, "startGame"):
                p.startGame()
        while self.game.getGameEnded(board, cur) == 0:
            it += 1
            if verbose:
                assert self.display
                print("Turn ", str(it), "Player ", str(cur))
                self.display(board)
            canonical = self.game.getCanonicalForm(board, cur)
            action = players[cur](canonical)
            valids = self.game.getValidMoves(self.game.getCanonicalForm(board, cur), 1)
            if valids[action] == 0:
                log.error(f"Action {action} is not valid!")
                log.debug(f"valids = {valids}")
                assert valids[action] > 0
            opponent = players[-cur]
            if hasattr(opponent, "notify"):
                opponent.notify(board, action)
            board, cur = self.game.getNextState(board, cur, action)
        for p in (self.player2, self.player1):
            if hasattr(p, "endGame"):
                p.endGame()
        if verbose:
            assert self.display
            print("Game over: Turn ", str(it), "Result ", str(self.game.getGameEnded(board, 1)))
            self.display(board)
        return cur * self.game.getGameEnded(board, cur)

    def playGamesForTwoPlayer(self, num, verbose=False):
        """num/2 games with player1 first, then num/2 with the roles swapped
        -> (player1 wins, player2 wins, draws) counted against the ORIGINAL player1."""
        num = int(num / 2)
        one = two = draws = 0
        for _ in tqdm(range(num), desc="Arena.playGames (Two-Player) (1)"):
            r = self.playGameForTwoPlayer(verbose=verbose)
            if r == 1:
                one += 1
            elif r == -1:
                two += 1
            else:
                draws += 1
        self.player1, self.player2 = self.player2, self.player1
        for _ in tqdm(range(num), desc="Arena.playGames (Two-Player) (2)"):
            r = self.playGameForTwoPlayer(verbose=verbose)
            if r == -1:
                one += 1
            elif r == 1:
                two += 1
            else:
                draws += 1
        return one, two, draws

    def playGames(self, num, verbose=False):
        if self.is_single_player:
            return self.playGamesForSinglePlayer(num, verbose)
        return self.playGamesForTwoPlayer(num, verbose)
