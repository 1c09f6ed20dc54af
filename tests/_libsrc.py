"""The source lists of the twelve libraries, once: binding module -> the files of its `X_ALLSRC =` line in deep_rl_amd/csrc/Makefile, in the Makefile's order and
relative to csrc/ (what csrc/srcid.py hashes into mi_x_source_id).  The test_*_abi_cpu.py files import their lists from here; test_ddqn_abi_cpu.py asserts that
every entry equals its Makefile line.  libmirl.so's list starts with the Makefile's own `$(SRCS)`, which SRCS below expands."""
INC = "../../include/"
SRCS = ["mi_env.hip", "mi_rollout.hip", "mi_update.hip", "mi_dqn.hip", "mi_sac.hip", "mi_comm.hip"]
# binding module -> the Makefile variable that holds its list
MAKE_VAR = {
    "_native": "ALLSRC", "_native_pg": "PG_ALLSRC", "_native_c51": "C51_ALLSRC", "_native_iqn": "IQN_ALLSRC", "_native_qr": "QR_ALLSRC",
    "_native_ddqn": "DDQN_ALLSRC", "_native_pdd": "PDD_ALLSRC", "_native_ns": "NS_ALLSRC", "_native_nz": "NZ_ALLSRC", "_native_rb": "RB_ALLSRC",
    "_native_ev": "EV_ALLSRC", "_native_md": "MD_ALLSRC",
}
ALLSRC = {
    "_native": ["$(SRCS)", "mi_common.h", "mi_grad_kernel.inc", "mi_sac_rowgroup.inc", INC + "mi_rl.h"],
    "_native_pg": ["mi_reinforce.hip", "mi_common.h", INC + "mi_reinforce.h", INC + "mi_rl.h"],
    "_native_c51": ["mi_c51.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", INC + "mi_c51.h", INC + "mi_rl.h"],
    "_native_iqn": ["mi_iqn.hip", "mi_common.h", "mi_ring.h", INC + "mi_iqn.h", INC + "mi_rl.h"],
    "_native_qr": ["mi_qr.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", INC + "mi_qr.h", INC + "mi_rl.h"],
    "_native_ddqn": ["mi_ddqn.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", "mi_qhead.h", INC + "mi_ddqn.h", INC + "mi_rl.h"],
    "_native_pdd": ["mi_pdd.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", "mi_dueling.h", INC + "mi_pdd.h", INC + "mi_rl.h"],
    "_native_ns": ["mi_nstep.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", "mi_nwalk.h", "mi_dueling.h", INC + "mi_nstep.h", INC + "mi_rl.h"],
    "_native_nz": ["mi_noisy.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", "mi_nwalk.h", "mi_dueling.h", INC + "mi_noisy.h", INC + "mi_rl.h"],
    "_native_rb": ["mi_rainbow.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", "mi_nwalk.h", INC + "mi_rainbow.h", INC + "mi_rl.h"],
    "_native_ev": ["mi_eval.hip", "mi_common.h", "mi_torso.h", INC + "mi_eval.h", INC + "mi_rl.h"],
    "_native_md": ["mi_mdqn.hip", "mi_common.h", "mi_ring.h", "mi_torso.h", "mi_qhead.h", INC + "mi_mdqn.h", INC + "mi_rl.h"],
}
