"""How many entry points and records include/crfconv_amd.h declares: the one place the host tests take the count from.  Update both
when the header changes.  (196 functions until three uncalled PointConv entries left the header, 193 until three uncalled SGD entries
did, 190 / 22 until the ragged-batch transforms' two entries and their spec record joined it.)"""
N_FUNCTIONS = 192
N_RECORDS = 23
