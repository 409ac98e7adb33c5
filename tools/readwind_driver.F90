! Driver of tools/make_golden_readwind.py: calls the reference's GRIB2WGRID (with its ADJUST, INCDATE and WSTREAM_STRG) on the records of a stream
! file and writes what it returns.  It is built by oracle/ref_build.py::build_driver: the routines and PARKIND_WAVE are the reference's own files,
! compiled unmodified in both precisions, behind the stand-ins of oracle/ref_stubs.F90 for what other packages supply.  One module is the driver's
! own, and the point of it: a YOWGRIB whose generic IGRIB_GET_VALUE / IGRIB_SET_VALUE answer integer, real, character, integer-array and
! real-array keys from a table this program fills from the file -- a stand-in for the GRIB decoder, not a decoder.  KRET is the optional fourth
! argument, which is also how the routine's positional IERR arrives: a key the table does not hold gives KRET = 1 where KRET is present and stops
! the program where it is not.
! READWIND and CURRENT2WAM are bound to files and to the message passing library, so their few statements on the field (readwind.F90:341-494,
! current2wam.F90:247-279) are restated here around the reference's FIELD.
! Input  (stream, little endian): NX, NY, NPTS (int32); KLONRGG(NY) (int32, south to north); IFROMIJ(NPTS), JFROMIJ(NPTS) (int32, 1-based); XLON(NX,NY),
!        YLAT(NX,NY), PMISS, ROAIR, WSTAR0, WLOWEST, CURRENT_MAX, SENTINEL (real64, representable in single precision); then records, each led by an
!        int32 OP (0 = the end):
!          1 GRIB2WGRID: POST, KRGG, LLWSWAVE, LLWDWAVE (int32); the key table: NI, NI x (name CHARACTER(40), int32); NR, NR x (name, real64); NS,
!                        NS x (name, CHARACTER(12)); NPL, PL(NPL) (int32; 0: no key 'pl'); NV, VALUES(NV) (real64)
!                        -> FIELD(NX,NY), IPARAM, IFORP, CDATE as a number, KZLEV.  POST = 1: READWIND's fill of FIELDG follows; POST = 2:
!                        CURRENT2WAM's statements on UCUR or VCUR follow
!          2 reset FIELDG(NX,NY,13) to SENTINEL, UCUR and VCUR(NPTS) to SENTINEL
!          3 -> FIELDG(NX,NY,13), UCUR(NPTS), VCUR(NPTS)
! Output (stream): per record the arrays listed, real64 (integers and working-precision results widened).
MODULE YOWGRIB
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  IMPLICIT NONE
  INTEGER(KIND=JWIM), PARAMETER :: JPGRIB_SUCCESS = 0
  INTEGER, PARAMETER :: MAXKEYS = 64
  ! the message: what the program read from the file
  INTEGER :: NIKEY = 0, NRKEY = 0, NSKEY = 0
  CHARACTER(LEN=40) :: CIKEY(MAXKEYS), CRKEY(MAXKEYS), CSKEY(MAXKEYS)
  INTEGER(KIND=JWIM) :: IKEYVAL(MAXKEYS)
  REAL(KIND=8) :: RKEYVAL(MAXKEYS)
  CHARACTER(LEN=12) :: SKEYVAL(MAXKEYS)
  INTEGER(KIND=JWIM), ALLOCATABLE :: PLVAL(:)
  REAL(KIND=8), ALLOCATABLE :: VALVAL(:)
  ! what the routine set
  REAL(KIND=JWRB) :: ZMISSING_SET = 0.0_JWRB
  CHARACTER(LEN=12) :: CSTEPUNITS_SET = ' '
  INTERFACE IGRIB_GET_VALUE
    MODULE PROCEDURE GET_INT, GET_REAL, GET_CHAR, GET_INT_ARRAY, GET_REAL_ARRAY
  END INTERFACE
  INTERFACE IGRIB_SET_VALUE
    MODULE PROCEDURE SET_CHAR, SET_REAL
  END INTERFACE
CONTAINS
  SUBROUTINE NOKEY(CDKEY, KRET)
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    IF (PRESENT(KRET)) THEN
      KRET = 1
    ELSE
      WRITE(0,*) 'readwind_driver: the message has no key ', CDKEY
      ERROR STOP 1
    ENDIF
  END SUBROUTINE NOKEY
  SUBROUTINE GET_INT(KHANDLE, CDKEY, KVAL, KRET)
    INTEGER(KIND=JWIM), INTENT(IN) :: KHANDLE
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY
    INTEGER(KIND=JWIM), INTENT(OUT) :: KVAL
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    INTEGER :: I
    KVAL = 0
    IF (PRESENT(KRET)) KRET = JPGRIB_SUCCESS
    DO I = 1, NIKEY
      IF (TRIM(CIKEY(I)) == CDKEY) THEN
        KVAL = IKEYVAL(I)
        RETURN
      ENDIF
    ENDDO
    CALL NOKEY(CDKEY, KRET)
  END SUBROUTINE GET_INT
  SUBROUTINE GET_REAL(KHANDLE, CDKEY, PVAL, KRET)
    INTEGER(KIND=JWIM), INTENT(IN) :: KHANDLE
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY
    REAL(KIND=JWRB), INTENT(OUT) :: PVAL
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    INTEGER :: I
    PVAL = 0.0_JWRB
    IF (PRESENT(KRET)) KRET = JPGRIB_SUCCESS
    DO I = 1, NRKEY
      IF (TRIM(CRKEY(I)) == CDKEY) THEN
        PVAL = REAL(RKEYVAL(I), JWRB)
        RETURN
      ENDIF
    ENDDO
    CALL NOKEY(CDKEY, KRET)
  END SUBROUTINE GET_REAL
  SUBROUTINE GET_CHAR(KHANDLE, CDKEY, CDVAL, KRET)
    INTEGER(KIND=JWIM), INTENT(IN) :: KHANDLE
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY
    CHARACTER(LEN=*), INTENT(OUT) :: CDVAL
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    INTEGER :: I
    CDVAL = ' '
    IF (PRESENT(KRET)) KRET = JPGRIB_SUCCESS
    DO I = 1, NSKEY
      IF (TRIM(CSKEY(I)) == CDKEY) THEN
        CDVAL = SKEYVAL(I)
        RETURN
      ENDIF
    ENDDO
    CALL NOKEY(CDKEY, KRET)
  END SUBROUTINE GET_CHAR
  SUBROUTINE GET_INT_ARRAY(KHANDLE, CDKEY, KVAL, KRET)
    INTEGER(KIND=JWIM), INTENT(IN) :: KHANDLE
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY
    INTEGER(KIND=JWIM), INTENT(OUT) :: KVAL(:)
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    IF (PRESENT(KRET)) KRET = JPGRIB_SUCCESS
    IF (CDKEY == 'pl' .AND. ALLOCATED(PLVAL)) THEN
      IF (SIZE(KVAL) /= SIZE(PLVAL)) ERROR STOP 2
      KVAL(:) = PLVAL(:)
    ELSE
      KVAL(:) = 0
      CALL NOKEY(CDKEY, KRET)
    ENDIF
  END SUBROUTINE GET_INT_ARRAY
  SUBROUTINE GET_REAL_ARRAY(KHANDLE, CDKEY, PVAL, KRET)
    INTEGER(KIND=JWIM), INTENT(IN) :: KHANDLE
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY
    REAL(KIND=JWRB), INTENT(OUT) :: PVAL(:)
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    IF (PRESENT(KRET)) KRET = JPGRIB_SUCCESS
    IF (CDKEY == 'values' .AND. ALLOCATED(VALVAL)) THEN
      IF (SIZE(PVAL) /= SIZE(VALVAL)) ERROR STOP 3
      PVAL(:) = REAL(VALVAL(:), JWRB)
    ELSE
      PVAL(:) = 0.0_JWRB
      CALL NOKEY(CDKEY, KRET)
    ENDIF
  END SUBROUTINE GET_REAL_ARRAY
  SUBROUTINE SET_CHAR(KHANDLE, CDKEY, CDVAL, KRET)
    INTEGER(KIND=JWIM), INTENT(IN) :: KHANDLE
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY, CDVAL
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    IF (PRESENT(KRET)) KRET = JPGRIB_SUCCESS
    IF (CDKEY == 'stepUnits') CSTEPUNITS_SET = CDVAL      ! the steps of the table are in seconds already
  END SUBROUTINE SET_CHAR
  SUBROUTINE SET_REAL(KHANDLE, CDKEY, PVAL, KRET)
    INTEGER(KIND=JWIM), INTENT(IN) :: KHANDLE
    CHARACTER(LEN=*), INTENT(IN) :: CDKEY
    REAL(KIND=JWRB), INTENT(IN) :: PVAL
    INTEGER(KIND=JWIM), OPTIONAL, INTENT(OUT) :: KRET
    IF (PRESENT(KRET)) KRET = JPGRIB_SUCCESS
    IF (CDKEY == 'missingValue') ZMISSING_SET = PVAL      ! the values of the table hold PMISS where they are missing already
  END SUBROUTINE SET_REAL
END MODULE YOWGRIB

PROGRAM READWIND_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWGRIB
  IMPLICIT NONE
#include "grib2wgrid.intfb.h"
  INTEGER, PARAMETER :: NFG = 13
  ! the planes of FIELDG in the order of ecwam_hip_forcing.h
  INTEGER, PARAMETER :: JUWND = 1, JVWND = 2, JAIRD = 3, JWSTAR = 4, JCICOVER = 5, JCITHICK = 6, JWSWAVE = 9, JWDWAVE = 10
  CHARACTER(LEN=512) :: FIN, FOUT
  INTEGER(KIND=JWIM) :: NX, NY, NPTS, OP, POST, KRGG, IWS, IWD, N, I, J, JSN, IJ, IX, JY
  INTEGER(KIND=JWIM) :: IFORP, IPARAM, KZLEV, KKK, MMM, KGRIB(1)
  INTEGER(KIND=JWIM), ALLOCATABLE :: KLONRGG(:), IFROMIJ(:), JFROMIJ(:)
  REAL(KIND=8) :: R8(6)
  REAL(KIND=8), ALLOCATABLE :: B2(:,:)
  REAL(KIND=JWRB) :: PMISS, ROAIR, WSTAR0, WLOWEST, CURRENT_MAX, SENT, ZDUM, RAD
  REAL(KIND=JWRB), ALLOCATABLE :: XLON(:,:), YLAT(:,:), FIELD(:,:), FIELDG(:,:,:), UCUR(:), VCUR(:)
  CHARACTER(LEN=14) :: CDATE
  REAL(KIND=8) :: DATE8

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(10, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(11, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(10) NX, NY, NPTS
  ALLOCATE(KLONRGG(NY), IFROMIJ(NPTS), JFROMIJ(NPTS), B2(NX,NY), XLON(NX,NY), YLAT(NX,NY), FIELD(NX,NY), FIELDG(NX,NY,NFG), UCUR(NPTS), VCUR(NPTS))
  READ(10) KLONRGG, IFROMIJ, JFROMIJ
  READ(10) B2
  XLON = REAL(B2, JWRB)
  READ(10) B2
  YLAT = REAL(B2, JWRB)
  READ(10) R8
  PMISS = REAL(R8(1), JWRB)
  ROAIR = REAL(R8(2), JWRB)
  WSTAR0 = REAL(R8(3), JWRB)
  WLOWEST = REAL(R8(4), JWRB)
  CURRENT_MAX = REAL(R8(5), JWRB)
  SENT = REAL(R8(6), JWRB)
  RAD = 4.0_JWRB*ATAN(1.0_JWRB)/180.0_JWRB
  FIELDG = SENT
  UCUR = SENT
  VCUR = SENT
  DO
    READ(10) OP
    IF (OP == 0) EXIT
    SELECT CASE (OP)
    CASE (1)
      READ(10) POST, KRGG, IWS, IWD
      READ(10) NIKEY
      DO I = 1, NIKEY
        READ(10) CIKEY(I), IKEYVAL(I)
      ENDDO
      READ(10) NRKEY
      DO I = 1, NRKEY
        READ(10) CRKEY(I), RKEYVAL(I)
      ENDDO
      READ(10) NSKEY
      DO I = 1, NSKEY
        READ(10) CSKEY(I), SKEYVAL(I)
      ENDDO
      IF (ALLOCATED(PLVAL)) DEALLOCATE(PLVAL)
      READ(10) N
      IF (N > 0) THEN
        ALLOCATE(PLVAL(N))
        READ(10) PLVAL
      ENDIF
      IF (ALLOCATED(VALVAL)) DEALLOCATE(VALVAL)
      READ(10) N
      ALLOCATE(VALVAL(N))
      READ(10) VALVAL
      ZDUM = 0.0_JWRB
      KGRIB(1) = 0
      ! as READWIND and CURRENT2WAM call it: LLCHKINT = .TRUE., the whole grid
      CALL GRIB2WGRID (6, 16, 1, KGRIB, 1, .FALSE., .TRUE., NY, KRGG, KLONRGG, 1, NX, 1, NY, XLON, YLAT, PMISS, ZDUM, ZDUM, &
 &                     CDATE, IFORP, IPARAM, KZLEV, KKK, MMM, FIELD)
      READ(CDATE, '(F14.0)') DATE8
      WRITE(11) REAL(FIELD, 8), REAL(IPARAM, 8), REAL(IFORP, 8), DATE8, REAL(KZLEV, 8)
      IF (POST == 1) THEN
        ! READWIND's fill (readwind.F90:341-494), restated: the loops end at NLONRGG_LOC(JSN)
        DO J = 1, NY
          JSN = NY-J+1
          DO I = 1, MIN(KLONRGG(JSN), NX)
            IF (IPARAM == 165 .OR. IPARAM == 33 .OR. IPARAM == 131 .OR. IPARAM == 180) THEN
              FIELDG(I,J,JUWND) = FIELD(I,J)
            ELSEIF (IPARAM == 166 .OR. IPARAM == 34 .OR. IPARAM == 132 .OR. IPARAM == 181) THEN
              FIELDG(I,J,JVWND) = FIELD(I,J)
            ELSEIF (IPARAM == 31 .OR. IPARAM == 139) THEN
              FIELDG(I,J,JCICOVER) = FIELD(I,J)
            ELSEIF (IPARAM == 92) THEN
              FIELDG(I,J,JCITHICK) = FIELD(I,J)
            ELSEIF (IPARAM == 245) THEN
              IF (IWS /= 0) THEN
                IF (FIELD(I,J) == PMISS) THEN
                  FIELDG(I,J,JWSWAVE) = 0.0_JWRB
                ELSE
                  FIELDG(I,J,JWSWAVE) = FIELD(I,J)
                ENDIF
              ENDIF
            ELSEIF (IPARAM == 249) THEN
              IF (IWD /= 0) THEN
                IF (FIELD(I,J) == PMISS) THEN
                  FIELDG(I,J,JWDWAVE) = 0.0_JWRB
                ELSE
                  FIELDG(I,J,JWDWAVE) = RAD*(FIELD(I,J)-180.0_JWRB)
                ENDIF
              ENDIF
            ELSEIF (IPARAM == 209) THEN
              IF (FIELD(I,J) == PMISS) THEN
                FIELDG(I,J,JAIRD) = ROAIR
              ELSE
                FIELDG(I,J,JAIRD) = FIELD(I,J)
              ENDIF
            ELSEIF (IPARAM == 208) THEN
              IF (FIELD(I,J) == PMISS) THEN
                FIELDG(I,J,JWSTAR) = WSTAR0
              ELSE
                FIELDG(I,J,JWSTAR) = FIELD(I,J)
              ENDIF
            ELSE
              ERROR STOP 4
            ENDIF
          ENDDO
        ENDDO
      ELSEIF (POST == 2) THEN
        ! CURRENT2WAM's statements (current2wam.F90:247-279), restated
        IF (IPARAM == 131 .OR. IPARAM == 140) THEN
          DO IJ = 1, NPTS
            IX = IFROMIJ(IJ)
            JY = JFROMIJ(IJ)
            UCUR(IJ) = FIELD(IX,JY)
            IF (ABS(UCUR(IJ)) <= WLOWEST) UCUR(IJ) = 0.0_JWRB
            IF (UCUR(IJ) <= PMISS) UCUR(IJ) = 0.0_JWRB
            UCUR(IJ) = SIGN(MIN(ABS(UCUR(IJ)),CURRENT_MAX),UCUR(IJ))
          ENDDO
        ELSEIF (IPARAM == 132 .OR. IPARAM == 139) THEN
          DO IJ = 1, NPTS
            IX = IFROMIJ(IJ)
            JY = JFROMIJ(IJ)
            VCUR(IJ) = FIELD(IX,JY)
            IF (ABS(VCUR(IJ)) <= WLOWEST) VCUR(IJ) = 0.0_JWRB
            IF (VCUR(IJ) <= PMISS) VCUR(IJ) = 0.0_JWRB
            VCUR(IJ) = SIGN(MIN(ABS(VCUR(IJ)),CURRENT_MAX),VCUR(IJ))
          ENDDO
        ELSE
          ERROR STOP 5
        ENDIF
      ENDIF
    CASE (2)
      FIELDG = SENT
      UCUR = SENT
      VCUR = SENT
    CASE (3)
      WRITE(11) REAL(FIELDG, 8), REAL(UCUR, 8), REAL(VCUR, 8)
    CASE DEFAULT
      ERROR STOP 6
    END SELECT
  ENDDO
  CLOSE(10)
  CLOSE(11)
END PROGRAM READWIND_DRIVER
